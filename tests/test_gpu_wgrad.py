"""Every weight-gradient tile form against torch-CPU float64, one case per kernel instantiation, reached by shape alone.

wgrad3x3.hip (all nine taps per workgroup, bf16 and split-bf16 "bf16x3"), wgrad_gemm2.hip (five bf16 tile forms, six bf16x3 ones) and
conv_wgrad.hip (the f32 kernel and the fixed-order slab reductions all three share).  No test here sets an environment switch.

Exact class (tolerance 0).  Operands for which fp32 accumulation is exact in ANY order, so the kernel must be bit-equal to float64:
  bf16 / f32 routes: x and dy hold integers from {-3, ..., 3}; every product and partial sum is an integer (quantum q = 1).
  bf16x3 route: x = a + b * 2^-8, a in {-3, -2, 2, 3}, b in {-1, 0, 1} (likewise dy), for which split() is asserted to return the
  planes (a, b * 2^-8) exactly.  The kernels keep hi*hi + hi*lo + lo*hi, so the exact result is W(dy_hi, x_hi) + W(dy_hi, x_lo) +
  W(dy_lo, x_hi), every term and partial sum a multiple of q = 2^-8.
  Condition, asserted per case before the launch: sum_m |dy| * |x| <= 2^22 * q for every dW entry (two bits under the 24-bit
  significand; the bf16 MFMA's order over its 16 products is not documented to round like successive fp32 adds).  The split class
  therefore needs M <= 1806 pixels; the one larger case (M = 17 340, the 256 x 256 split tile) runs the integer class with both lo planes
  zero, its lo-plane addressing is left to the random class.
  A dropped or doubled dy * x product shows as a difference of 4 q or more in one tap.

Random class.  randn operands at the project's existing tolerances: close(..., X3_TOL) for bf16x3, tol(float32, ref) for f32, and
rtol = atol / max|ref| = 2e-3 for bf16 on bf16-rounded operands.  err / bound is printed per case.

Per case, on the same operands: the route (nslices and slab_elems of the recorded reduction descriptor against the tables below, which
restate wg3_th / wg3x_th / wgrad3x3(_x3)_slices, wg2_pick, wg2x_pick and pick_wgrad; the descriptor is the authority on what ran),
deferred == immediate bit for bit, and a second immediate call bit-equal to the first.

Section 1: 3x3 / stride 1 / pad 1 on wgrad3x3_kernel (single band, ragged last slices 3 + 2, 3 + 3 + 1 and a last slice of one band,
           image boundaries and halo rows inside a slice, 8 and 9 slabs: wgrad_reduce<4> at its limit and wgrad_reduce<16>).
Section 2: everything else on wgrad_gemm2_kernel / wgrad_kernel<float>, every tile form including 64(co) x 128(ci), with M ragged against
           the 16-, 32- and 64-row steps and a short last slice in every multi-slice case.
Section 3: accumulate onto a slice of a larger flat buffer, and the workspace bound with a guarded 4 KiB tail, once per kernel family.
Section 4: a split-bf16 launch of 2^21 or more output pixels through the deferred entry point (two half-batches over one workspace).
Section 5: the grouped launch (ab_conv2d_wgrad_x3_group) on the split exact class, different operands per problem: the problem select, the
           per-problem slab pointers and the ragged last slice of every problem; and G = 1 through it bit-equal to ab_conv2d_wgrad_x3.

Observed on an MI355X.
  Exact class: all 105 (case, route) pairs of sections 1 and 2, the five accumulate cases and the six exact-size workspaces are bit-equal
  to float64 (34 on the split class, the rest on the integer class); nothing was found.  Every descriptor agrees with the tables.
  Largest err / bound of the random class:
    section 1  bf16 7.6e-05 ((7, 8, 16, 64, 128))   bf16x3 0.230 ((1, 4, 32, 64, 64))          f32 0.036 ((7, 8, 16, 64, 128))
    section 2  bf16 8.4e-05 ((11, 13, 9, 64, 128, 3, 1, 1))   bf16x3 0.207 ((3, 14, 10, 128, 64, 3, 2, 1))   f32 0.030 ((17, 34, 30, 256, 320, 1, 1, 0))
  (bf16 on bf16-rounded operands leaves only the fp32 summation order: its 2e-3 allowance is 10^4 times what the kernels need, which is why
  the exact class carries the bf16 route.)
  Section 3: the bf16x3 launches fill ab_conv2d_wgrad_x3_workspace to the byte (7, 6 and 68 slabs); the bf16 / f32 ones use 0.3 - 0.9 MB
  of the 75.8 MB ab_conv2d_wgrad_workspace promises.
  Section 4: immediate vs the float64 sum of the halves 2.4e-4 (bound 5.7e-2).  Before the fix in conv_x3.hip / conv_wgrad.hip the deferred
  call differed from the immediate one by 3.8e+3 at max|dw| = 5.7e+3 (it kept out's contents plus the second half only).
  Section 5: all seven problems of the three grouped cases and both groups of one are bit-equal to float64; nothing was found.
"""
import ctypes
import functools
import types

import pytest
import torch

from test_gpu_conv import tol
from test_gpu_conv_x3 import X3_TOL, close, nchw

pytestmark = pytest.mark.gpu

BF16, F32, X3 = "bf16", "f32", "x3"
SPLIT_MAX_M = 1806          # (3 * 3 + 2 * 3 * 2^-8 + slack: 9.07) * M * 2^8 <= 2^22


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- cases
# (a) 3x3 / stride 1 / pad 1: (N, H, W, Cin, Cout), then per route what the dispatch rules give.
#     bf16, bf16x3: (nbands, bands_per_slice, slices) of wgrad3x3_kernel; bf16 None: the all-taps kernel declines (wg3_th) and wgrad_gemm2 runs
#     <64,64> with the (slices, rows_per_slice) given.   f32: (BI x BJ, slices, rows_per_slice) of wgrad_kernel<float>.
A_CASES = [
    ((1, 2, 64, 64, 64), (1, 1, 1), (2, 2, 1), ("64x64", 1, 128)),          # single band; the double buffer never flips
    ((3, 2, 64, 64, 64), (3, 3, 1), (6, 2, 3), ("64x64", 1, 384)),          # W = 64 forms; image boundaries inside a slice
    ((1, 6, 64, 64, 128), (3, 3, 1), (6, 2, 3), ("128x64", 1, 384)),        # bands inside one image: halo rows are real data
    ((1, 4, 32, 64, 64), (1, 1, 1), (2, 2, 1), ("64x64", 1, 128)),          # W = 32 single band
    ((5, 4, 32, 64, 64), (5, 3, 2), (10, 2, 5), ("64x64", 1, 640)),         # ragged last slice (3 + 2)
    ((3, 4, 32, 128, 64), (3, 3, 1), (6, 2, 3), ("64x128", 1, 384)),        # two ci tiles
    ((1, 8, 16, 64, 64), (1, 1, 1), (2, 2, 1), ("64x64", 1, 128)),          # W = 16 single band
    ((7, 8, 16, 64, 128), (7, 3, 3), (14, 2, 7), ("128x64", 1, 896)),       # last slice of ONE band; two co tiles
    ((3, 16, 16, 64, 64), (6, 2, 3), (12, 2, 6), ("64x64", 1, 768)),        # two / four bands per image
    ((1, 8, 8, 64, 64), (1, 1, 1), (1, 1, 1), ("64x64", 1, 64)),            # W = 8: 16 k-rows span two image rows
    ((5, 8, 8, 128, 192), (5, 3, 2), (5, 3, 2), ("64x128", 1, 320)),        # 2 x 3 tiles (a co / ci tile swap shows)
    ((7, 8, 8, 64, 64), (7, 3, 3), (7, 3, 3), ("64x64", 1, 448)),           # 3 + 3 + 1
    ((18, 8, 8, 64, 64), (18, 2, 9), (18, 2, 9), ("64x64", 2, 576)),        # 9 slabs: wgrad_reduce<16>
    ((4, 16, 16, 64, 64), (8, 2, 4), (16, 2, 8), ("64x64", 1, 1024)),       # bf16x3: 8 slabs, wgrad_reduce<4> at its limit (bf16: want 256 > 8 / 2)
    ((19, 8, 8, 64, 64), (19, 3, 7), (19, 3, 7), ("64x64", 2, 608)),        # last slice of one band
    ((1, 1, 64, 64, 64), None, (1, 1, 1), ("64x64", 1, 64)),                # split TH = 1, one row
    ((5, 2, 32, 64, 64), None, (5, 3, 2), ("64x64", 1, 320)),               # split TH = 2
    ((7, 4, 16, 64, 64), None, (7, 3, 3), ("64x64", 1, 448)),               # split TH = 4
]
A_GEMM2 = {(1, 1, 64, 64, 64): (1, 64), (5, 2, 32, 64, 64): (1, 320), (7, 4, 16, 64, 64): (1, 448)}
WG3_TH = {BF16: {64: 2, 32: 4, 16: 8, 8: 8}, X3: {64: 1, 32: 2, 16: 4, 8: 8}}

# (b) (N, H, W, Cin, Cout, k, stride, pad), M, then (BI x BJ, slices, rows_per_slice) for bf16 (wg2_pick), bf16x3 (wg2x_pick), f32 (pick_wgrad)
B_CASES = [
    ((3, 14, 10, 64, 64, 3, 2, 1), 105, ("64x64", 1, 128), ("64x64", 1, 128), ("64x64", 1, 128)),
    ((3, 14, 10, 128, 64, 3, 2, 1), 105, ("64x128", 1, 128), ("64x128", 1, 128), ("64x128", 1, 128)),
    ((3, 14, 10, 64, 128, 3, 2, 1), 105, ("128x64", 1, 128), ("128x64", 1, 128), ("128x64", 1, 128)),
    ((3, 14, 10, 128, 128, 3, 2, 1), 105, ("128x128", 1, 128), ("128x128", 1, 128), ("128x128", 1, 128)),
    ((3, 14, 10, 256, 128, 3, 2, 1), 105, ("128x256", 1, 128), ("128x128", 1, 128), ("128x128", 1, 128)),
    ((3, 14, 10, 128, 256, 3, 2, 1), 105, ("128x128", 1, 128), ("256x128", 1, 128), ("128x128", 1, 128)),
    ((5, 22, 14, 128, 64, 1, 2, 0), 385, ("64x128", 1, 448), ("64x128", 2, 224), ("64x128", 1, 416)),
    ((7, 12, 14, 128, 64, 4, 2, 1), 294, ("64x128", 1, 320), ("64x128", 2, 160), ("64x128", 1, 320)),       # sixteen taps
    ((5, 13, 9, 128, 64, 1, 1, 0), 585, ("64x128", 2, 320), ("64x128", 3, 224), ("64x128", 1, 608)),
    ((9, 13, 9, 64, 64, 3, 1, 1), 1053, ("64x64", 3, 384), ("64x64", 5, 224), ("64x64", 2, 544)),          # nine taps, padding on all four sides
    ((11, 13, 9, 128, 64, 3, 1, 1), 1287, ("64x128", 3, 448), ("64x128", 6, 224), ("64x128", 2, 672)),
    ((11, 13, 9, 64, 128, 3, 1, 1), 1287, ("128x64", 3, 448), ("128x64", 6, 224), ("128x64", 2, 672)),
    ((9, 13, 9, 128, 128, 1, 1, 0), 1053, ("128x128", 3, 384), ("128x128", 5, 224), ("128x128", 2, 544)),
    ((5, 13, 9, 256, 128, 1, 1, 0), 585, ("128x256", 2, 320), ("128x128", 3, 224), ("128x128", 1, 608)),
    ((9, 13, 9, 128, 256, 1, 1, 0), 1053, ("128x128", 3, 384), ("256x128", 5, 224), ("128x128", 2, 544)),
    ((9, 13, 9, 64, 192, 1, 1, 0), 1053, ("64x64", 3, 384), ("64x64", 5, 224), ("64x64", 2, 544)),
    ((17, 34, 30, 256, 320, 1, 1, 0), 17340, ("64x128", 34, 512), ("256x256", 68, 256), ("64x128", 17, 1024)),   # bf16x3: partial last co tile
]
# the template arguments wgrad_gemm2_run / wgrad_gemm2_x3_run launch for a tile
GEMM2_FORM = {BF16: {"128x256": "128_256_w8", "128x128": "128_128_w8", "128x64": "128_64_w8", "64x128": "64_128_w8", "64x64": "64_64"},
              X3: {"256x256": "256_256_2stage", "256x128": "256_128", "128x128": "128_128", "128x64": "128_64", "64x128": "64_128",
                   "64x64": "64_64"}}


def _a_params():
    out = []
    for shape, b, x, f in A_CASES:
        case = shape + (3, 1, 1)
        N, H, W, Cin, Cout = shape
        sid = "x".join(map(str, shape))
        if b is not None:
            out.append(pytest.param(case, BF16, b, id=f"bf16-wg3_{W}_{WG3_TH[BF16][W]}_8-{sid}"))
        else:
            out.append(pytest.param(case, BF16, ("64x64",) + A_GEMM2[shape], id=f"bf16-gemm2_64_64-{sid}"))
        out.append(pytest.param(case, X3, x, id=f"x3-wg3_{W}_{WG3_TH[X3][W]}_8_x3-{sid}"))
        out.append(pytest.param(case, F32, f, id=f"f32-wgrad_float_{f[0].replace('x', '_')}-{sid}"))
    return out


def _b_params():
    out = []
    for case, M, b, x, f in B_CASES:
        N, H, W, Cin, Cout, k, s, p = case
        assert M == N * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
        sid = "x".join(map(str, case))
        out.append(pytest.param(case, BF16, b, id=f"bf16-gemm2_{GEMM2_FORM[BF16][b[0]]}-{sid}"))
        out.append(pytest.param(case, X3, x, id=f"x3-gemm2_{GEMM2_FORM[X3][x[0]]}_x3-{sid}"))
        out.append(pytest.param(case, F32, f, id=f"f32-wgrad_float_{f[0].replace('x', '_')}-{sid}"))
    return out


# ---------------------------------------------------------------- operands and float64 references (computed once, shared, never written to)
def _geom(case):
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    return Ho, Wo, N * Ho * Wo


def _w64(case, x, dy):
    """float64 weight gradient of NHWC operands, as [Cout][kh][kw][Cin]."""
    N, H, W, Cin, Cout, k, s, p = case
    return torch.nn.grad.conv2d_weight(nchw(x).double(), (Cout, Cin, k, k), nchw(dy).double(), stride=s, padding=p).permute(0, 2, 3, 1).contiguous()


def _seed(case, salt):
    return salt + sum(v * 31 ** i for i, v in enumerate(case)) % (1 << 31)


@functools.lru_cache(maxsize=None)
def _exact(case, cls, salt=1):
    """cls 'int': integers from {-3..3}, q = 1.  cls 'split': a + b * 2^-8, q = 2^-8, with the planes split() must return.
    salt: another draw of the same class (the problems of a grouped launch)."""
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo, M = _geom(case)
    g = torch.Generator().manual_seed(_seed(case, salt))
    o = types.SimpleNamespace(cls=cls)

    def draw(shape):
        if cls == "int":
            hi = torch.randint(-3, 4, shape, generator=g).float()
            return hi, torch.zeros(shape)
        hi = torch.tensor([-3.0, -2.0, 2.0, 3.0])[torch.randint(0, 4, shape, generator=g)]
        return hi, torch.randint(-1, 2, shape, generator=g).float() * 2.0 ** -8

    o.xh, o.xl = draw((N, H, W, Cin))
    o.dh, o.dl = draw((N, Ho, Wo, Cout))
    o.x, o.dy = o.xh + o.xl, o.dh + o.dl                       # exact in fp32: 10 significant bits
    o.q = 1.0 if cls == "int" else 2.0 ** -8
    # hi*hi + hi*lo + lo*hi; float64 holds every one of these sums exactly
    o.ref, mass = _w64(case, o.x, o.dh), _w64(case, o.xh.abs() + o.xl.abs(), o.dh.abs())
    if cls == "split":
        o.ref, mass = o.ref + _w64(case, o.xh, o.dl), mass + _w64(case, o.xh.abs(), o.dl.abs())
    o.mass = float(mass.max())                                 # max over dW of sum_m |dy| * |x| over the plane pairs the kernels keep
    return o


@functools.lru_cache(maxsize=None)
def _random(case, rounded):
    """randn operands (rounded to bf16 for the bf16 route, so that both sides see the same inputs) and their float64 weight gradient."""
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo, M = _geom(case)
    g = torch.Generator().manual_seed(_seed(case, 2))
    o = types.SimpleNamespace()
    o.x, o.dy = torch.randn((N, H, W, Cin), generator=g), torch.randn((N, Ho, Wo, Cout), generator=g)
    if rounded:
        o.x, o.dy = o.x.to(torch.bfloat16).float(), o.dy.to(torch.bfloat16).float()
    o.ref = _w64(case, o.x, o.dy)
    return o


def _device_operands(route, x, dy, planes=None):
    """The tensors K.conv2d_wgrad(_x3) takes for a route; planes: the (xh, xl, dh, dl) split() must return exactly."""
    from artiboost_amd import kernels as K
    if route == BF16:
        xb, db = x.to(torch.bfloat16), dy.to(torch.bfloat16)
        assert torch.equal(xb.float(), x) and torch.equal(db.float(), dy)
        return xb.cuda(), db.cuda()
    if route == F32:
        return x.cuda(), dy.cuda()
    xs, ds = K.split(x.cuda()), K.split(dy.cuda())
    if planes is not None:
        for got, want in zip((xs[0], xs[1], ds[0], ds[1]), planes):
            assert torch.equal(got.float().cpu(), want), "split() does not return the planes the exact class is built on"
    return xs, ds


def _call(route, xd, dd, case, **kw):
    from artiboost_amd import kernels as K
    N, H, W, Cin, Cout, k, s, p = case
    return (K.conv2d_wgrad_x3 if route == X3 else K.conv2d_wgrad)(xd, dd, k, k, s, p, **kw)


def _assert_exact(what, got, ref, q):
    """Bit-equality with the float64 result; on failure say how many entries differ, by how many quanta, and where."""
    got = got.double().cpu()
    if torch.equal(got, ref):
        return
    d = (got - ref) / q
    bad = d.nonzero()
    first = ", ".join(f"(co {int(a)}, tap {int(b) * ref.shape[2] + int(c)}, ci {int(e)}): {float(d[a, b, c, e]):+g} q" for a, b, c, e in bad[:6])
    whole = bool((d == d.round()).all())
    raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} entries differ, largest {float(d.abs().max()):g} q"
                         f"{'' if whole else ' (NOT all multiples of q: the exactness premise fails)'}; first: {first}")


def _ratio(route, got, ref):
    """err / bound at the project's existing tolerance of the route (printed by the caller, asserted here)."""
    got = got.double().cpu()
    err = (got - ref).abs()
    if route == X3:
        r = float(err.max()) / (X3_TOL * (float(ref.abs().max()) + 1e-30))
        close(got, ref)
        return r
    t = tol(torch.float32, ref) if route == F32 else dict(rtol=2e-3, atol=2e-3 * float(ref.abs().max()))
    r = float((err / (t["atol"] + t["rtol"] * ref.abs())).max())
    assert r <= 1.0, f"{route}: err / bound {r:.3f} (max err {float(err.max()):.3e}, max|ref| {float(ref.abs().max()):.3e})"
    return r


def _expected_slices(case, route, expect):
    """The table's slice count, after checking the table row against itself."""
    N, H, W, Cin, Cout, k, s, p = case
    M = _geom(case)[2]
    if isinstance(expect[0], str):                                  # (BI x BJ, slices, rows_per_slice)
        tile, ns, rows = expect
        bi, bj = map(int, tile.split("x"))
        assert cdiv(M, rows) == ns and rows % 32 == 0 and (k * k * Cin) % bj == 0 and (Cout % bi == 0 or (route == X3 and bi == 256)), (case, expect)
        return ns
    nbands, bps, ns = expect                                        # wgrad3x3_kernel
    assert (k, s, p) == (3, 1, 1) and nbands == N * (H // WG3_TH[route][W]) and cdiv(nbands, bps) == ns, (case, expect)
    return ns


def _check(case, route, expect, section):
    from artiboost_amd import kernels as K
    N, H, W, Cin, Cout, k, s, p = case
    M = _geom(case)[2]
    ns = _expected_slices(case, route, expect)
    slab = Cout * k * k * Cin

    # ---- exact class
    e = _exact(case, "split" if route == X3 and M <= SPLIT_MAX_M else "int")
    assert e.mass <= 2.0 ** 22 * e.q, f"exactness condition: sum |dy||x| = {e.mass:g} > 2^22 q"
    xd, dd = _device_operands(route, e.x, e.dy, (e.xh, e.xl, e.dh, e.dl))
    pend = K.PendingReductions()
    deferred = _call(route, xd, dd, case, defer=pend)
    d = pend.descs[-1]
    print(f"wgrad s{section} {route} {case}: descriptor nslices {d.nslices} slab_elems {d.slab_elems}; table {expect}; exact class '{e.cls}' "
          f"mass {e.mass / e.q:.0f} q of {2 ** 22}")
    assert (d.nslices, d.slab_elems) == (ns, slab), f"route: the launch recorded {d.nslices} slabs of {d.slab_elems}, the table has {ns} of {slab}"
    pend.flush()
    now = _call(route, xd, dd, case)
    again = _call(route, xd, dd, case)
    _assert_exact(f"{route} {case}", now, e.ref, e.q)
    assert torch.equal(deferred, now), "deferred reduction != immediate call"
    assert torch.equal(again, now), "a second immediate call differs"

    # ---- random class
    r = _random(case, route == BF16)
    xd, dd = _device_operands(route, r.x, r.dy)
    pend = K.PendingReductions()
    deferred = _call(route, xd, dd, case, defer=pend)
    assert (pend.descs[-1].nslices, pend.descs[-1].slab_elems) == (ns, slab)
    pend.flush()
    now = _call(route, xd, dd, case)
    ratio = _ratio(route, now, r.ref)
    print(f"wgrad s{section} {route} {case}: random class err / bound {ratio:.3e}")
    assert torch.equal(deferred, now), "deferred reduction != immediate call (random class)"
    assert torch.equal(_call(route, xd, dd, case), now), "a second immediate call differs (random class)"


# ---------------------------------------------------------------- 1. the all-taps 3x3 / stride 1 kernel
@pytest.mark.parametrize("case,route,expect", _a_params())
def test_wgrad3x3_forms(case, route, expect):
    _check(case, route, expect, 1)


# ---------------------------------------------------------------- 2. wgrad_gemm2_kernel / wgrad_kernel<float>, every tile form
@pytest.mark.parametrize("case,route,expect", _b_params())
def test_wgrad_gemm_forms(case, route, expect):
    _check(case, route, expect, 2)


# ---------------------------------------------------------------- 3. accumulate and the workspace bound, once per kernel family
C3 = (7, 8, 16, 64, 128, 3, 1, 1)            # wgrad3x3_kernel: 3 slices (bf16), 7 (bf16x3); wgrad_kernel<float, 128, 64>
G2 = (11, 13, 9, 128, 64, 3, 1, 1)           # wgrad_gemm2_kernel 64 x 128: 3 slices (bf16), 6 (bf16x3)
BIG = (17, 34, 30, 256, 320, 1, 1, 0)        # 256 x 256 split tile whose last co tile holds 64 of 256 rows: 68 slabs end at the buffer's end
FAMILIES = [pytest.param(C3, BF16, id="bf16-wgrad3x3"), pytest.param(C3, X3, id="x3-wgrad3x3"), pytest.param(G2, BF16, id="bf16-gemm2"),
            pytest.param(G2, X3, id="x3-gemm2"), pytest.param(C3, F32, id="f32-wgrad_kernel")]


@pytest.mark.parametrize("case,route", FAMILIES)
def test_accumulate_onto_a_slice_of_a_flat_buffer(case, route):
    """accumulate=True adds the exact result to what out holds and writes nothing else of the buffer out is a slice of."""
    N, H, W, Cin, Cout, k, s, p = case
    e = _exact(case, "split" if route == X3 else "int")
    assert e.mass + 8 <= 2.0 ** 22 * e.q
    xd, dd = _device_operands(route, e.x, e.dy)
    n, pre, post = e.ref.numel(), 260, 1028
    g = torch.Generator().manual_seed(5)
    flat0 = torch.randint(-8, 9, (pre + n + post,), generator=g).float()
    flat = flat0.cuda()
    out = flat[pre:pre + n].view(Cout, k, k, Cin)
    res = _call(route, xd, dd, case, out=out, accumulate=True)
    assert res.data_ptr() == out.data_ptr()
    got = flat.cpu()
    _assert_exact(f"accumulate {route} {case}", got[pre:pre + n].view(Cout, k, k, Cin), flat0[pre:pre + n].view(Cout, k, k, Cin).double() + e.ref, e.q)
    assert torch.equal(got[:pre], flat0[:pre]) and torch.equal(got[pre + n:], flat0[pre + n:]), "wrote outside out"


@pytest.mark.parametrize("case,route", FAMILIES + [pytest.param(BIG, X3, id="x3-gemm2-partial-co-tile")])
def test_workspace_bound_and_guarded_tail(case, route):
    """The slabs a launch records fit the bytes ab_conv2d_wgrad(_x3)_workspace promises, and a direct deferred call on a buffer of exactly
    that size leaves a 4 KiB tail of 0xA5 behind it unchanged."""
    from artiboost_amd import _lib as L
    from artiboost_amd import kernels as K
    N, H, W, Cin, Cout, k, s, p = case
    M = _geom(case)[2]
    lib = L.lib()
    e = _exact(case, "split" if route == X3 and M <= SPLIT_MAX_M else "int")
    assert e.mass <= 2.0 ** 22 * e.q
    xd, dd = _device_operands(route, e.x, e.dy)
    if route == X3:
        nbytes = lib.ab_conv2d_wgrad_x3_workspace(L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(k), L.i(k), L.i(s), L.i(p))
    else:
        nbytes = lib.ab_conv2d_wgrad_workspace(L.i(M), L.i(Cout), L.i(k * k * Cin))
    pend = K.PendingReductions()
    _call(route, xd, dd, case, defer=pend)
    d = pend.descs[-1]
    print(f"wgrad s3 {route} {case}: {d.nslices} slabs x {d.slab_elems * 4} bytes = {d.nslices * d.slab_elems * 4} of {nbytes}")
    assert 0 < d.nslices * d.slab_elems * 4 <= nbytes
    pend.flush()

    TAIL = 4096
    buf = torch.full((nbytes + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    dw = torch.empty((Cout, k, k, Cin), dtype=torch.float32, device="cuda")
    desc = L.WgradReduceDesc()
    if route == X3:
        L.check(lib.ab_conv2d_wgrad_x3_deferred(L.ptr(xd[0]), L.ptr(xd[1]), L.ptr(dd[0]), L.ptr(dd[1]), L.ptr(dw), L.i(N), L.i(H), L.i(W), L.i(Cin),
                                                L.i(Cout), L.i(k), L.i(k), L.i(s), L.i(p), L.ptr(buf), L.i(0), ctypes.byref(desc), L.stream()),
                "ab_conv2d_wgrad_x3_deferred")
    else:
        L.check(lib.ab_conv2d_wgrad_deferred(L.ptr(xd), L.ptr(dd), L.ptr(dw), L.i(L.dt(xd)), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout), L.i(k),
                                             L.i(k), L.i(s), L.i(p), L.ptr(buf), L.i(0), ctypes.byref(desc), L.stream()), "ab_conv2d_wgrad_deferred")
    assert desc.nslices == d.nslices and desc.slabs == buf.data_ptr()
    L.check(lib.ab_wgrad_reduce_batch((L.WgradReduceDesc * 1)(desc), L.i(1), L.stream()), "ab_wgrad_reduce_batch")
    assert bool((buf[nbytes:] == 0xA5).all()), "the launch wrote behind its workspace"
    _assert_exact(f"exact-size workspace {route} {case}", dw, e.ref, e.q)


# ---------------------------------------------------------------- 4. 2^21 or more output pixels through the deferred entry point
def test_wgrad_x3_deferred_beyond_2p21_pixels():
    """A split-bf16 weight gradient over 2^21 or more output pixels runs as two half-batches over ONE workspace, so a deferred call cannot
    record it as one reduction: it reduces both halves itself (nslices == 0) and gives the immediate call's bits.  (1x1, 64 -> 64, batch
    130 at 128 x 128; about 2.2 GB on the device.)"""
    from artiboost_amd import kernels as K
    N, H, W, C = 130, 128, 128, 64
    assert N * H * W >= 1 << 21
    g = torch.Generator(device="cuda").manual_seed(1)
    x = K.split(torch.randn((N, H, W, C), generator=g, device="cuda"))
    dy = K.split(torch.randn((N, H, W, C), generator=g, device="cuda"))
    dw = K.conv2d_wgrad_x3(x, dy, 1, 1, 1, 0)
    h = N // 2
    ref = torch.zeros((C, 1, 1, C), dtype=torch.float64, device="cuda")
    for sl in (slice(0, h), slice(h, N)):
        ref += K.conv2d_wgrad_x3(x[:, sl].contiguous(), dy[:, sl].contiguous(), 1, 1, 1, 0).double()
    err, scale = float((dw.double() - ref).abs().max()), float(ref.abs().max())
    print(f"wgrad s4: immediate vs sum of the halves: err {err:.3e}, bound {1e-5 * scale:.3e}")
    assert err <= 1e-5 * scale
    pend = K.PendingReductions()
    out = torch.full((C, 1, 1, C), 7.0, device="cuda")            # a deferred call that loses the first half also keeps what dw held
    deferred = K.conv2d_wgrad_x3(x, dy, 1, 1, 1, 0, out=out, defer=pend)
    pend.flush()
    assert torch.equal(deferred, dw), f"deferred != immediate: max diff {float((deferred - dw).abs().max()):.3e} (max|dw| {scale:.3e})"


# ---------------------------------------------------------------- 5. the grouped launch of wgrad3x3_kernel
# (N, H, W, Cin, Cout), G, then (nbands, bands_per_slice, slices PER PROBLEM): wgrad3x3_x3_group_slices aims at 256 / (tiles * G) slices, which
# the two-bands-per-slice clamp (nbands / 2) cuts to the single launch's count at these sizes
GROUP_CASES = [((7, 8, 8, 64, 64), 2, (7, 3, 3)), ((7, 8, 8, 64, 64), 3, (7, 3, 3)),      # 3 + 3 + 1 bands per problem
               ((5, 8, 8, 128, 192), 2, (5, 3, 2))]                                         # 2 x 3 tiles


@pytest.mark.parametrize("shape,G,expect", [pytest.param(s, G, e, id=f"G{G}-" + "x".join(map(str, s))) for s, G, e in GROUP_CASES])
def test_wgrad3x3_group_exact(shape, G, expect):
    """Every problem of a grouped launch bit-equal to float64 on its own operands, the slot behind the last problem untouched, a second call
    bit-equal to the first."""
    from artiboost_amd import _lib as L
    from artiboost_amd import kernels as K
    case = shape + (3, 1, 1)
    N, H, W, Cin, Cout = shape
    ns = _expected_slices(case, X3, expect)
    assert _geom(case)[2] <= SPLIT_MAX_M
    nbytes = L.lib().ab_conv2d_wgrad_x3_group_workspace(L.i(G), L.i(N), L.i(H), L.i(W), L.i(Cin), L.i(Cout))
    assert nbytes == G * ns * Cout * 9 * Cin * 4, f"route: workspace of {nbytes} bytes, the table has {G} x {ns} slabs"
    flat = torch.full((G + 1, Cout, 3, 3, Cin), 7.0, device="cuda")
    es = [_exact(case, "split", salt=3 + i) for i in range(G)]
    assert not torch.equal(es[0].x, es[1].x) and not torch.equal(es[0].dy, es[1].dy)
    items = []
    for i, e in enumerate(es):
        assert e.mass <= 2.0 ** 22 * e.q, f"exactness condition: sum |dy||x| = {e.mass:g} > 2^22 q"
        xd, dd = _device_operands(X3, e.x, e.dy, (e.xh, e.xl, e.dh, e.dl))
        items.append((xd, dd, flat[i]))
    K.conv2d_wgrad_x3_group(items)
    for i, e in enumerate(es):
        _assert_exact(f"group of {G}, problem {i}, {case}", flat[i], e.ref, e.q)
    assert bool((flat[G] == 7.0).all()), "wrote behind the last problem"
    again = torch.full_like(flat, 7.0)
    K.conv2d_wgrad_x3_group([(a, b, again[i]) for i, (a, b, _) in enumerate(items)])
    assert torch.equal(again, flat), "a second grouped call differs"


@pytest.mark.parametrize("shape", [(3, 2, 64, 64, 64), (7, 8, 16, 64, 128)], ids=lambda s: "x".join(map(str, s)))
def test_wgrad3x3_group_of_one_equals_the_single_launch(shape):
    """G = 1 through ab_conv2d_wgrad_x3_group gives ab_conv2d_wgrad_x3's bits (and float64's) on the same operands."""
    from artiboost_amd import kernels as K
    case = shape + (3, 1, 1)
    e = _exact(case, "split")
    assert e.mass <= 2.0 ** 22 * e.q, f"exactness condition: sum |dy||x| = {e.mass:g} > 2^22 q"
    xd, dd = _device_operands(X3, e.x, e.dy, (e.xh, e.xl, e.dh, e.dl))
    single = _call(X3, xd, dd, case)
    out = torch.full_like(single, 7.0)
    K.conv2d_wgrad_x3_group([(xd, dd, out)])
    _assert_exact(f"group of one {case}", out, e.ref, e.q)
    assert torch.equal(out, single), "a group of one differs from the single launch"
