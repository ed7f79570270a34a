"""The eval-mode kernels that fold a BatchNorm into the convolution before it, each against torch-CPU float64, one case per tile form.

Every number the project reports comes from the eval-mode forward, which in bf16x3 runs ab_conv2d_fwd_x3_evalbn (conv3x3.hip, X3 = 3, eight
tile configurations), ab_conv2d_fwd_x3_affine (convp.hip or the generic epilogue), ab_conv2d_dgrad_x3_affine (conv2x2.hip's transposed
forward at 32x32 and at four 16x16 images per tile, or the generic four-parity-class kernel) and ab_bn_eval_params(_batch).  No test here
sets an environment switch: each tile form is reached by shape alone, the way the model reaches it.

Tolerance.  X3_TOL (tests/test_gpu_conv_x3.py) bounds the error of a bf16x3 convolution relative to the largest output.  The affine map
carries it to  X3_TOL * (max|scale| * max|conv_ref| + max|res|)  (ReLU is 1-Lipschitz).  It is deliberately NOT taken relative to
max|ref_out|: shift and residual can cancel against the convolution.

Headroom of the reference side (test_evalbn_operand_split_headroom, computed on the CPU in float64): with the operands replaced by their
(hi, lo) bf16 planes and the three products the kernels keep (hi*hi + hi*lo + lo*hi), the error against the exact float64 result is at most
0.096 of that bound over all twelve shapes (0.071 to 0.096; worst: (37, 56, 56, 64, 64)).  What remains of the bound belongs to the kernel's fp32 accumulation
over 9 * Cin terms (about sqrt(9 * Cin) * 2^-24 of the output scale when rounding errors do not line up: 0.05 of the bound at Cin = 64).

Largest observed error / bound on an MI355X:
  section 1 (conv2d_fwd_x3_evalbn, cfg 1-8)                 0.131  (cfg 4, (2, 12, 20, 64, 40), no residual, ReLU; cfg 7: 0.096; cfg 8 seam, image 1: 0.130)
  section 2 (refused shapes: conv2d_fwd_x3 + bn_apply_x3)   0.136  ((1, 12, 8, 64, 128), no residual, no ReLU)
  section 3 (conv2d_dgrad_x3_affine; conv2d_fwd_x3_affine)  0.199  ((2, 14, 14, 64, 32) on the generic four-class kernel; patch kernels 0.133 - 0.169; forward 0.167)
  section 4 (bn_eval_params_batch, in units of its 2^-21)   0.306  (shift at C = 512; scale 0.270, invstd 0.197)
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_x3 import X3_TOL, nhwc

pytestmark = pytest.mark.gpu


def _bn_state(C, g):
    """Non-trivial BatchNorm state: gamma U(0.5, 1.5), beta 0.3 randn, running_mean 0.1 randn, running_var U(0.5, 1.5)."""
    return (torch.rand(C, generator=g) + 0.5, 0.3 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g),
            torch.rand(C, generator=g) + 0.5)


def _ratio(what, got, ref, bound):
    """Print, then assert: max|got - ref| <= bound.  Returns err / bound."""
    err = float((got.double() - ref).abs().max())
    print(f"eval_fold {what}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.4f}")
    assert err <= bound, f"{what}: max err {err:.3e} > bound {bound:.3e} (ratio {err / bound:.3f})"
    return err / bound


def _same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------- 1. conv2d_fwd_x3_evalbn, one case per tile instantiation
# (cfg, (N, H, W, Cin, Cout)): the configuration c3_config chooses for a plain bf16x3 launch of that shape
EVALBN = [
    (4, (2, 12, 20, 64, 40)),       # tw = 16 partial in W, th = 8 partial in H, ragged 40-channel n-tile
    (4, (1, 8, 32, 64, 64)),        # the W >= 24 route to cfg 4
    (1, (1, 10, 24, 96, 64)),       # Cin % 64 == 32; partial tiles both ways
    (2, (1, 9, 28, 64, 136)),       # second n-tile holds 8 channels
    (3, (1, 14, 14, 64, 72)),       # ragged n-tile, partial H
    (6, (1, 16, 16, 64, 128)),      # whole-image tile
    (6, (1, 16, 12, 64, 64)),       # ... with W < tw
    (5, (3, 7, 7, 64, 128)),        # odd N at <= 8x8 must not stack
    (5, (1, 8, 8, 64, 72)),
    (8, (2, 8, 8, 64, 128)),        # stacked pairs of 8x8 images
    (8, (4, 8, 8, 128, 192)),
]
CFG7 = (37, 56, 56, 64, 64)         # N * ceil(H / 8) * ceil(W / 32) = 518 >= 512: the 256-pixel x 64-channel tile


def _sid(p):
    form, shape = p
    return (f"cfg{form}-" if isinstance(form, int) else f"{form}-") + "x".join(map(str, shape))


@functools.lru_cache(maxsize=None)
def _conv_case(shape, img0_scale=1.0):
    """One 3x3/s1/p1 layer + BatchNorm + residual: the float64 reference (computed once, shared, never written to) and the device operands.
    scale64 / shift64 are the DEVICE's bnp rows 0 and 1, so that these tests isolate the convolution and its epilogue."""
    from artiboost_amd import kernels as K
    N, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(1000 * N + 100 * H + 10 * W + Cin + Cout)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, 3, 3), generator=g) * (2.0 / (Cin * 9)) ** 0.5
    gam, bet, rm, rv = _bn_state(Cout, g)
    r = torch.randn((N, Cout, H, W), generator=g)
    if img0_scale != 1.0:
        x[0] *= img0_scale
        r[0] *= img0_scale
    c = types.SimpleNamespace(shape=shape, x=x, w=w)
    c.conv64 = nhwc(F.conv2d(x.double(), w.double(), padding=1))
    c.xd = nhwc(x).cuda()
    c.ws = K.split(w.permute(0, 2, 3, 1).contiguous().cuda())                    # OHWI
    c.bnp = K.bn_eval_params(gam.cuda(), bet.cuda(), rm.cuda(), rv.cuda())
    c.scale64, c.shift64 = c.bnp[0].double().cpu(), c.bnp[1].double().cpu()
    c.res_planes = K.split(nhwc(r).cuda())
    c.res_f32 = c.res_planes[0].float() + c.res_planes[1].float()                # the fp32 tensor hi + lo of those same planes
    c.r64 = c.res_f32.double().cpu()
    return c


def _ref_and_bound(c, res, relu, img=slice(None)):
    ref = c.conv64[img] * c.scale64 + c.shift64
    bound = float(c.scale64.abs().max()) * float(c.conv64[img].abs().max())
    if res:
        ref = ref + c.r64[img]
        bound += float(c.r64[img].abs().max())
    return (ref.clamp_min(0) if relu else ref), X3_TOL * bound


C3_TILE = {1: (4, 32), 2: (8, 32), 3: (8, 16), 4: (8, 16), 5: (8, 8), 6: (16, 16), 7: (8, 32)}      # cfg -> (rows, columns) of its pixel tile


def _assert_cfg(cfg, shape):
    """The configuration is reached by shape: the launch's BatchNorm-partial row count is its spatial tile count (cfg 8: one per image pair).
    (1 and 7 differ in the tile's height; 2 / 7 and 3 / 4 share a pixel tile and differ in Cout <= 64.)"""
    from artiboost_amd import _lib as L
    N, H, W, Cin, Cout = shape
    rows = L.lib().ab_conv2d_x3_stat_rows(L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(3), L.i(3), L.i(1), L.i(1))
    th, tw = C3_TILE.get(cfg, (0, 0))
    assert rows == (N // 2 if cfg == 8 else N * -(-H // th) * -(-W // tw)), (cfg, shape, rows)
    assert cfg == 6 or (Cout <= 64) == (cfg in (1, 4, 7))


def _check_evalbn(cfg, c, res_kind, relu, what):
    from artiboost_amd import kernels as K
    assert K.conv2d_fwd_x3_evalbn_ok(c.xd, c.ws)
    _assert_cfg(cfg, c.shape)
    res = {"none": None, "planes": c.res_planes, "f32": c.res_f32}[res_kind]
    got = K.conv2d_fwd_x3_evalbn(c.xd, c.ws, c.bnp, res=res, relu=relu, want_f32=True)
    ref, bound = _ref_and_bound(c, res is not None, relu)
    ratio = _ratio(what, got.cpu(), ref, bound)
    # planes match fp32; want_f32 changes nothing in the planes
    sp = got._ab_split
    assert _same(sp, K.split(got)), "planes != split(fp32 output)"
    assert _same(K.conv2d_fwd_x3_evalbn(c.xd, c.ws, c.bnp, res=res, relu=relu, want_f32=False), sp), "want_f32 changes the planes"
    # the header's contract: bit-identical to the convolution and ab_bn_apply_x3 as separate launches
    two = K.bn_apply_x3(K.conv2d_fwd_x3(c.xd, c.ws, 1, 1), c.bnp, res=res, relu=relu, want_f32=True)
    assert _same(got, two), "fold != conv2d_fwd_x3 + bn_apply_x3 (fp32)"
    assert _same(sp, two._ab_split), "fold != conv2d_fwd_x3 + bn_apply_x3 (planes)"
    if res_kind == "f32":       # the residual's form is irrelevant
        alt = K.conv2d_fwd_x3_evalbn(c.xd, c.ws, c.bnp, res=c.res_planes, relu=relu, want_f32=True)
        assert _same(got, alt) and _same(sp, alt._ab_split), "residual as fp32 != residual as planes"
    return got, ratio


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "norelu"])
@pytest.mark.parametrize("res_kind", ["none", "planes", "f32"])
@pytest.mark.parametrize("case", EVALBN, ids=_sid)
def test_evalbn_matches_float64_per_tile_config(case, res_kind, relu):
    _check_evalbn(case[0], _conv_case(case[1]), res_kind, relu, f"S1 {_sid(case)} res={res_kind} relu={int(relu)}")


def test_evalbn_cfg7_256_pixel_tile_matches_float64():
    """The smallest shape-only route to the 256 x 64 tile (layer 1 of an evaluation at B >= 37); planes residual, ReLU."""
    _check_evalbn(7, _conv_case(CFG7), "planes", True, f"S1 {_sid((7, CFG7))} res=planes relu=1")


@pytest.mark.parametrize("res_kind", ["none", "planes"])
def test_evalbn_cfg8_stacked_pair_does_not_leak_across_the_seam(res_kind):
    """cfg 8 runs images 2k and 2k+1 as one 16-row image.  Image 0 at 1e4 scale beside image 1 at unit scale: image 1's output must match its
    float64 reference at image 1's OWN scale -- one row of image 0 read across the seam would be 1e4 times the bound."""
    from artiboost_amd import kernels as K
    c = _conv_case((2, 8, 8, 64, 128), 1e4)
    res = c.res_planes if res_kind == "planes" else None
    got = K.conv2d_fwd_x3_evalbn(c.xd, c.ws, c.bnp, res=res, relu=True, want_f32=True).cpu()
    for img in (0, 1):
        ref, bound = _ref_and_bound(c, res is not None, True, img=slice(img, img + 1))
        _ratio(f"S1 seam res={res_kind} image {img}", got[img:img + 1], ref, bound)


@pytest.mark.parametrize("case", EVALBN + [(7, CFG7)], ids=_sid)
def test_evalbn_operand_split_headroom(case):
    """Reference side only (CPU, float64): the operands as (hi, lo) bf16 planes and the three products the kernels keep, against the exact
    convolution.  It must use at most a quarter of the bound; the rest is for the fp32 accumulation on the device (module docstring)."""
    c = _conv_case(case[1])

    def planes(t):
        hi = t.bfloat16()
        return hi.double(), (t - hi.float()).bfloat16().double()
    (xh, xl), (wh, wl) = planes(c.x), planes(c.w)
    emu = nhwc(F.conv2d(xh, wh, padding=1) + F.conv2d(xh, wl, padding=1) + F.conv2d(xl, wh, padding=1))
    ref, bound = _ref_and_bound(c, True, True)
    ratio = _ratio(f"S1-headroom {_sid(case)}", (emu * c.scale64 + c.shift64 + c.r64).clamp_min(0), ref, bound)
    assert ratio <= 0.25


# ---------------------------------------------------------------- 2. the predicate and its refusals
REFUSED = [
    (1, 8, 8, 64, 64),        # W <= 8 needs Cout > 64
    (1, 10, 10, 64, 128),     # 9 <= W <= 11
    (1, 4, 4, 64, 128),
    (1, 12, 8, 64, 128),      # H > 8 at W <= 8
    (1, 16, 16, 64, 68),      # Cout % 8 != 0
    (1, 16, 16, 48, 64),      # Cin % 32 != 0
]


@pytest.mark.parametrize("shape", REFUSED, ids=lambda s: "x".join(map(str, s)))
def test_evalbn_predicate_is_false_and_the_kernel_refuses_without_writing(shape):
    from artiboost_amd import _lib as L, kernels as K
    c = _conv_case(shape)
    N, H, W, Cin, Cout = shape
    assert not K.conv2d_fwd_x3_evalbn_ok(c.xd, c.ws)
    with pytest.raises(RuntimeError, match="ab_conv2d_fwd_x3_evalbn failed with code -2"):
        K.conv2d_fwd_x3_evalbn(c.xd, c.ws, c.bnp, res=c.res_planes, relu=True, want_f32=True)
    # the wrapper allocates its outputs: poisoned buffers through the library binding
    xh, xl = K._planes(c.xd)
    out = torch.full((2, N, H, W, Cout), 123.0, dtype=torch.bfloat16, device="cuda")
    out_f = torch.full((N, H, W, Cout), 123.0, dtype=torch.float32, device="cuda")
    try:
        rc = L.lib().ab_conv2d_fwd_x3_evalbn(L.ptr(xh), L.ptr(xl), L.ptr(c.ws[0]), L.ptr(c.ws[1]), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout),
                                             L.ptr(c.bnp), L.ptr(c.res_planes[0]), L.ptr(c.res_planes[1]), L.ptr(None), L.i(1), L.ptr(out[0]),
                                             L.ptr(out[1]), L.ptr(out_f), L.stream())
    except RuntimeError as e:          # the torch-op binding raises on a non-zero return code; the ctypes binding returns it
        assert "code -2" in str(e), e
        rc = -2
    assert rc == -2                    # AB_ESHAPE
    with pytest.raises(RuntimeError, match="code -2"):
        L.check(rc, "ab_conv2d_fwd_x3_evalbn")
    torch.cuda.synchronize()
    assert bool((out == 123.0).all()) and bool((out_f == 123.0).all()), "a refused launch wrote to its outputs"


@pytest.mark.parametrize("res_kind,relu", [("planes", True), ("none", False)])
@pytest.mark.parametrize("shape", REFUSED, ids=lambda s: "x".join(map(str, s)))
def test_refused_shapes_have_a_correct_two_launch_route(shape, res_kind, relu):
    """Where the predicate says no, HybridNet._eval_block runs conv2d_fwd_x3 + bn_apply_x3: that route against float64."""
    from artiboost_amd import kernels as K
    c = _conv_case(shape)
    res = c.res_planes if res_kind == "planes" else None
    got = K.bn_apply_x3(K.conv2d_fwd_x3(c.xd, c.ws, 1, 1), c.bnp, res=res, relu=relu, want_f32=True)
    ref, bound = _ref_and_bound(c, res is not None, relu)
    _ratio(f"S2 {'x'.join(map(str, shape))} res={res_kind} relu={int(relu)}", got.cpu(), ref, bound)
    assert _same(got._ab_split, K.split(got))


# ---------------------------------------------------------------- 3a. conv2d_dgrad_x3_affine: ConvTranspose2d(4x4, s2, p1) + BN + ReLU
# (form, (N, H_out, W_out, C output channels, K input channels))
TCONV = [
    ("patch32", (1, 32, 32, 64, 64)),
    ("patch32", (1, 32, 32, 128, 32)),        # the 128-wide n-tile with K = 32
    ("patch32", (2, 32, 32, 192, 64)),        # 192 -> 64-wide tiles
    ("patch16x4", (4, 16, 16, 64, 64)),       # four images per tile (image 0 at 1e4 scale, see the test)
    ("patch16x4", (8, 16, 16, 128, 32)),
    ("generic4", (3, 16, 16, 64, 64)),        # N % 4 != 0
    ("generic4", (2, 14, 14, 64, 32)),
    ("generic4", (1, 12, 20, 36, 32)),        # a channel count that is a multiple of 4 only
]


@functools.lru_cache(maxsize=None)
def _tconv_case(shape, img0_scale=1.0):
    """Weights and BatchNorm state depend on (H, W, C, K) only and the input is drawn image by image, so the N = 3 case is the first three
    images of the N = 4 case with the same layer."""
    from artiboost_amd import kernels as K
    N, H, W, C, Kc = shape
    g = torch.Generator().manual_seed(100 * H + 10 * W + C + Kc)
    w = torch.randn((Kc, C, 4, 4), generator=g) * (2.0 / (Kc * 16)) ** 0.5       # ConvTranspose2d weight [in, out, kh, kw]
    gam, bet, rm, rv = _bn_state(C, g)
    x = torch.stack([torch.randn((Kc, H // 2, W // 2), generator=g) for _ in range(N)])
    if img0_scale != 1.0:
        x[0] *= img0_scale
    c = types.SimpleNamespace(shape=shape)
    c.conv64 = nhwc(F.conv_transpose2d(x.double(), w.double(), stride=2, padding=1))
    c.dy = nhwc(x).cuda()
    c.wt = K.split(w.permute(1, 2, 3, 0).contiguous().cuda())                   # [C][kh][kw][K]: dgrad (IHWO) layout of the mirrored conv
    c.bnp = K.bn_eval_params(gam.cuda(), bet.cuda(), rm.cuda(), rv.cuda())
    c.scale64, c.shift64 = c.bnp[0].double().cpu(), c.bnp[1].double().cpu()
    c.r64 = None
    return c


def _tconv_run(c):
    from artiboost_amd import kernels as K
    N, H, W, C, Kc = c.shape
    sp = K.conv2d_dgrad_x3_affine(c.dy, c.wt, (H, W), 2, 1, c.bnp, relu=True)
    assert sp.shape == (2, N, H, W, C)
    return sp, (sp[0].double() + sp[1].double()).cpu()


@pytest.mark.parametrize("case", TCONV, ids=_sid)
def test_tconv_affine_matches_float64_and_the_two_launch_route(case):
    from artiboost_amd import _lib as L, kernels as K
    form, shape = case
    N, H, W, C, Kc = shape
    rows = L.lib().ab_conv2d_dgrad_x3_stat_rows(L.i(N), L.i(H), L.i(W), L.i(C), L.i(Kc), L.i(4), L.i(4), L.i(2), L.i(1))
    if form == "patch32":           # the form is reached by shape: conv2x2_tfwd_rows is N * 4 at 32x32, N at 16x16 with N % 4 == 0
        assert rows == N * 4
    elif form == "patch16x4":
        assert rows == N
    scaled = shape == (4, 16, 16, 64, 64)
    c = _tconv_case(shape, 1e4 if scaled else 1.0)
    sp, got = _tconv_run(c)
    ref, bound = _ref_and_bound(c, False, True)
    _ratio(f"S3 {_sid(case)}", got, ref, bound)
    if scaled:      # a mix-up between the four images of a tile shows at the unit-scale images' own scale
        for img in range(1, N):
            ref, bound = _ref_and_bound(c, False, True, img=slice(img, img + 1))
            _ratio(f"S3 {_sid(case)} image {img}", got[img:img + 1], ref, bound)
    two = K.bn_apply_x3(K.conv2d_dgrad_x3(c.dy, c.wt, (H, W), 2, 1), c.bnp, relu=True)
    assert _same(sp, two), "fold != conv2d_dgrad_x3 + bn_apply_x3"


def test_tconv_affine_generic_and_patch_kernels_agree():
    """(3, 16, 16, 64, 64) on the generic four-class kernel == the first three images of the N = 4 run of the patch kernel, within the bound."""
    c3, c4 = _tconv_case((3, 16, 16, 64, 64)), _tconv_case((4, 16, 16, 64, 64))
    assert torch.equal(c3.dy, c4.dy[:3]) and torch.equal(c3.wt, c4.wt) and torch.equal(c3.bnp, c4.bnp)
    _, g3 = _tconv_run(c3)
    _, g4 = _tconv_run(c4)
    ref, bound = _ref_and_bound(c4, False, True)
    _ratio("S3 patch16x4 unscaled", g4, ref, bound)
    _, bound3 = _ref_and_bound(c3, False, True)
    _ratio("S3 generic4 vs patch16x4", g3, g4[:3], bound3)


# ---------------------------------------------------------------- 3b. conv2d_fwd_x3_affine on the generic epilogue
# ((N, H, W, Cin, Cout), k, stride, pad): the forms the issue names are (relu, planes) = (False, False) for the 1x1, (True, True) for the 3x3
FWD_AFFINE = [
    ((2, 16, 16, 64, 128), 1, 2, 0),          # the downsample branch of _eval_block
    ((3, 14, 10, 64, 128), 1, 2, 0),
    ((2, 9, 5, 64, 72), 1, 1, 0),
    ((3, 14, 10, 64, 128), 3, 2, 1),          # Cin = 64 is not the patch kernel's shape
]


@pytest.mark.parametrize("case", FWD_AFFINE, ids=lambda c: "x".join(map(str, c[0])) + f"-k{c[1]}s{c[2]}p{c[3]}")
def test_fwd_affine_generic_epilogue_matches_float64(case):
    from artiboost_amd import kernels as K
    (N, H, W, Cin, Cout), k, s, p = case
    g = torch.Generator().manual_seed(N + H + W + Cout + 7 * k)
    x = torch.randn((N, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, k, k), generator=g) * (2.0 / (Cin * k * k)) ** 0.5
    gam, bet, rm, rv = _bn_state(Cout, g)
    xd = nhwc(x).cuda()
    ws = K.split(w.permute(0, 2, 3, 1).contiguous().cuda())
    bnp = K.bn_eval_params(gam.cuda(), bet.cuda(), rm.cuda(), rv.cuda())
    c = types.SimpleNamespace(conv64=nhwc(F.conv2d(x.double(), w.double(), stride=s, padding=p)), scale64=bnp[0].double().cpu(),
                              shift64=bnp[1].double().cpu())
    out = {(relu, planes): K.conv2d_fwd_x3_affine(xd, ws, bnp, s, p, relu=relu, planes=planes) for relu in (False, True) for planes in (False, True)}
    what = "S3 fwd_affine " + "x".join(map(str, case[0])) + f" k{k}s{s}"
    for relu in (False, True):
        ref, bound = _ref_and_bound(c, False, relu)
        _ratio(f"{what} relu={int(relu)} fp32", out[relu, False].cpu(), ref, bound)
        sp = out[relu, True]
        _ratio(f"{what} relu={int(relu)} planes", (sp[0].double() + sp[1].double()).cpu(), ref, bound)
        assert _same(sp, K.split(out[relu, False])), "planes != split(fp32 output)"
    assert _same(out[True, False], out[False, False].clamp_min(0)), "relu=True != clamp_min(relu=False, 0)"


# ---------------------------------------------------------------- 4. bn_eval_params and bn_eval_params_batch
def test_bn_eval_params_batch_rows_offsets_padding_and_float64():
    from artiboost_amd import kernels as K
    eps = 1e-5
    Cs = [1, 8, 64, 72, 300, 512]
    g = torch.Generator().manual_seed(38)
    state = [list(_bn_state(C, g)) for C in Cs]
    state[4][3][7], state[4][3][299] = 0.0, 1e6          # running_var = 0 (invstd = eps^-1/2) and 1e6
    # gamma / beta in `flat`, mean / var in `stats`, every tensor at a NON-monotone offset with other data between them, so that a swapped
    # descriptor column reads another tensor (or another BatchNorm's) rather than a neighbour with similar values
    order_flat = [(i, j) for j in (1, 0) for i in (3, 0, 5, 2, 4, 1)]
    order_stats = [(i, j) for i in (2, 5, 1, 4, 0, 3) for j in (3, 2)]
    off, flat_parts, stats_parts = {}, [], []
    for order, parts, pad in ((order_flat, flat_parts, 3), (order_stats, stats_parts, 5)):
        pos = pad
        parts.append(torch.full((pad,), 7.0))
        for i, j in order:
            off[i, j] = pos
            parts += [state[i][j], torch.full((pad,), 7.0)]
            pos += Cs[i] + pad
    flat, stats = torch.cat(flat_parts).cuda(), torch.cat(stats_parts).cuda()
    desc, out_off = [], 0
    for i, C in enumerate(Cs):
        desc.append((off[i, 0], off[i, 1], off[i, 2], off[i, 3], out_off, C))
        out_off += 4 * ((C + 63) // 64 * 64)
    out = torch.full((out_off,), float("nan"), device="cuda")
    K.bn_eval_params_batch(flat, stats, torch.tensor(desc, dtype=torch.int32).cuda(), len(Cs), max(Cs), out, eps=eps)
    out = out.cpu()
    worst = 0.0
    for (_, _, _, _, o, C), (gam, bet, rm, rv) in zip(desc, state):
        row = out[o:o + 4 * C].view(4, C)
        one = K.bn_eval_params(gam.cuda(), bet.cuda(), rm.cuda(), rv.cuda(), eps=eps).cpu()
        assert torch.equal(row, one), f"C = {C}: the batched row differs from ab_bn_eval_params"
        assert bool(torch.isnan(out[o + 4 * C:o + 4 * ((C + 63) // 64 * 64)]).all()), f"C = {C}: padding behind the row was written"
        invstd = 1.0 / torch.sqrt(rv.double() + eps)
        scale = gam.double() * invstd
        shift = bet.double() - rm.double() * scale
        u = 2.0 ** -21
        assert bool(torch.isfinite(row).all())
        rel = torch.stack([((row[0].double() - scale) / scale).abs().max(), ((row[3].double() - invstd) / invstd).abs().max(),
                           ((row[1].double() - shift).abs() / (bet.double().abs() + (rm.double() * scale).abs())).max()]) / u
        print(f"eval_fold S4 C={C}: scale {float(rel[0]):.3f} invstd {float(rel[1]):.3f} shift {float(rel[2]):.3f} (units of 2^-21)")
        worst = max(worst, float(rel.max()))
        assert float(rel[0]) <= 1.0 and float(rel[1]) <= 1.0, f"C = {C}: scale / invstd off by {rel[:2].tolist()} x 2^-21"
        assert float(rel[2]) <= 1.0, f"C = {C}: shift off by {float(rel[2])} x 2^-21 (|beta| + |mean * scale|)"
        assert torch.equal(row[2], rm), f"C = {C}: mean is not the running mean"
    print(f"eval_fold S4 worst: ratio {worst:.4f}")
