"""Every BatchNorm, pooling and packing kernel form of norm_pool.hip against torch-CPU float64, reached by shape alone at the defaults.

No test here sets an environment switch.  Shapes are (M, C) or (N, H, W, C); dtypes 'f32' (4 channels per lane) and 'bf16' (8 per lane).
The reference is plain torch on the CPU in float64, written from the definitions: biased batch variance (the running variance takes the
unbiased one), bnp = (scale, shift, mean, invstd), out = relu?(y * scale + shift [+ res | + res_y * scale2 + shift2]), dz = dout * mask,
dbeta = sum dz, dgamma = sum dz * xhat, dy = scale * (dz - dbeta / M - xhat * dgamma / M), and the 3x3 / 2 / pad 1 max-pool with the FIRST
maximum in scan order (winner code dh * 3 + dw relative to (2 ho - 1, 2 wo - 1)), taken from F.max_pool2d(return_indices=True) in float64
and asserted equal to a written-out strict-greater scan on every tied input used.  Planes are compared with K.split of the float64 result
rounded to fp32, bit for bit.

Exact class (tolerance 0).  y = mu_c + sigma_c * s with integer mu_c in {-3..3}, sigma_c in {1/2, 1, 2}, s = +-1 balanced per channel
  where the statistics feed a finalize (M even): mean = mu_c and var = sigma_c^2 exactly, eps = 0, invstd in {2, 1, 1/2}, gamma in
  {-2, -1, 1, 2}, beta an odd multiple of 1/2, integer residual (a BatchNorm-ed residual has an integer beta), so the pre-activation is an
  odd multiple of 1/2 and never 0.  Momentum 1/2 or 1/4 with dyadic initial running statistics: running_mean exact, running_var within
  1 ulp of fp32 (one fp32 multiply-add of a correctly rounded double).  Per channel sum |y| and sum y^2 over a launch <= 2^22, asserted per
  case: partial rows and bnp are bit-equal to float64 in any summation order.  Backward: integer dout in {-3..3}, xhat = +-1, so dgamma,
  dbeta and bwdp are exact integers for every M; dy is exact where M is a power of two (invM exact) and goes to the bound of the random
  class otherwise.  The same y makes nearly every pool window tie.  Every exact launch is repeated and must be bit-equal to itself.
Random class.  randn operands with a per-channel offset and scale.  The bound is computed per case in float64 from the inputs: an fp32 sum
  of L terms in a fixed serial order is within (L - 1) u sum |x_i| of the exact one (u = 2^-24, first order); the longest chain of the
  reductions here is the per-lane row loop (ceil(rows / rl) terms) followed by the rl-term LDS combine, L = ceil(rows / rl) + rl, and the
  finalize is in double.  stats_bound gives (L u sum |x|, (L + 1) u sum x^2), bnp_bound carries it through mean, var, invstd, scale and
  shift, apply_bound to out, bwd_bound to dgamma / dbeta / dy (an element whose pre-activation is within its own rounding of 0 may take
  either mask value: its |dout| is added to the bound instead of guessing).  The assertion is err <= 4 x bound (MARGIN, for the terms
  the first-order model drops); err / bound is printed per case.

Form table (the tables below carry it per case; tests/test_bn_pool_host.py checks it against the restated dispatchers):
  section 1  col_stats<f32|bf16> (vc, rl) incl. vc = 24 / rl = 10 (C = 96 f32), vc = 5 / rl = 51 (C = 40 bf16), vc = 1, vc = 256,
             red_rows 16 and 32, one-row last block; col_stats_x3; colsum_finalize; the AB_ESHAPE refusals
  section 2  reduce_parts_1024<8>: tail loop only (nparts <= 128), 2-deep loop (129 .. 896), 8-deep loop (> 896); c < C guard (C = 4, 12,
             100); count = 1; running statistics absent; variance clamp; bn_bwd_finalize through ab_bn_bwd_apply
  section 3  bn_apply / bn_bwd_reduce / bn_bwd_apply <f32|bf16>, fixed and per-iteration parameters, ysl = 2, grid wrap on both paths
  section 4  bn_apply_x3<false>, <true>, <false, true>, bn_apply_x3_c4 (no / fp32 / plane residual), wraps; bn_fin_apply_x3<0 / 1 / 2>
             (nparts % 4 != 0, M < 32, M % 32 != 0, nsl = 32, strip wrap, one running-statistics update); ab_bn_bwd_x3 on the in-kernel
             finalize and on finalize + apply with four mask sources, given rows, ysl = 2
  section 5  maxpool_fwd / bwd <f32|bf16>, maxpool_fwd<float> + planes (C % 8 == 4), maxpool_fwd_x3 (+ ywin, out = NULL),
             bn_bwd_reduce / apply with pool_idx, pool_bwd_bn_reduce<8, false> + pool_bwd_bn_apply_x3, pool_win_bn_reduce, and the
             route hybridnet.py takes where ab_bn_relu_maxpool_bwd_x3_nparts == 0 (max-pool backward + bn_bwd_x3 recompute)
  section 6  avgpool_fwd <f32|bf16>, relu_bwd, add, cast_f32_bf16, transpose_oki, image_pad_nhwc4
  section 7  guarded 4 KiB tails of 0xA5, once per kernel family

Not reachable by shape: bn_finalize_kernel<2> / <4> and bn_bwd_finalize_kernel<2> / <4> (AB_BNFIN_CPW only); pool_bwd_bn_reduce_kernel<4, *>,
  <16, *> (AB_PBR_RP) and <8, true> (AB_POOL_BWD_REGATHER=0, which also is the only caller of bn_bwd_apply_x3_kernel with a premasked dz
  from the pool); maxpool_fwd_kernel<float> + planes at C % 8 == 0 (AB_POOL_FWD_V8=0 or idx = NULL); bn_bwd_reduce_kernel<bf16_t> with
  gridDim.y = 2 needs C = 4096 in bf16, which no model has (the f32 form of the same code is in the table).  None is in the tables.

Observed on an MI355X.
  Exact class: all 2892 exact comparisons of the file (partial rows, totals, bnp, running_mean, out, planes, winners, ywin, dz, dgamma,
  dbeta, bwdp, dy at power-of-two M, the packing kernels; 260 tests) are bit-equal to float64, every repeated launch is bit-equal to
  the first, running_var is within its 1 ulp everywhere, every row count agrees with the restated formulas, every refusal returns
  AB_ESHAPE with its outputs untouched, and no guarded byte changed.
  Largest err / bound (bound = the first-order bound, before the factor 4):
    section 3  0.972  bn_bwd<bf16> (1000, 96), every relu: dy stored in bf16 (the 2^-8 store rounding is the whole bound and is reached)
               0.333  bn_bwd<f32> (16386, 512) relu=1 res: dy;   random class 0.314  (4096, 64) relu=1: dy,  0.244  (4096, 64): out
    section 4  0.489  bn_bwd_x3 grid wrap (174764, 96): dy (hi + lo);   random class 0.478  (520, 1024): dy (hi + lo)
    section 5  0.929  pool<bf16> (2, 10, 6, 64): dy stored in bf16;   0.443  pool x3w (2, 10, 6, 64): dy (hi + lo)
    section 6  0.168  avgpool_fwd<f32> randn (3, 49, 132)
  Relative error of invstd at C = 64, M = 4096 (first-order bound in brackets): |mean| / std = 0: 4.8e-8 (6.3e-7); 8: 6.6e-7 (1.1e-4);
    64: 4.6e-5 (6.7e-3) -- the cancellation of sum x^2 / M - mean^2 costs three decimal digits between ratio 0 and 64; the bound
    allows four.
  Wall time of the file: 14 s (the four grid-wrap cases take 1.4 - 3.5 s each, every other case under 0.4 s).
  Sensitivity: against a build of norm_pool.hip with four planted errors (maxpool_fwd_x3 keeping the LAST maximum, every strip of
  bn_fin_apply_x3 updating the running statistics, bn_apply taking its fixed-channel shortcut at every C, the 2-deep loop of
  reduce_parts_1024 dropping its second load) 63 of the 260 tests fail, in every section that launches one of the four.
  Found and changed: nothing.  No kernel, dispatcher or wrapper differs from its reference at any form in the tables.
"""
import functools
import re
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LIM = 2.0 ** 22
MARGIN = 4.0
ESHAPE = -2
F32, BF16 = "f32", "bf16"
TD = {F32: torch.float32, BF16: torch.bfloat16}
VEC = {F32: 4, BF16: 8}
WRAP_VECS = 8192 * 256          # grid_for caps the grid at 8192 workgroups of 256 lanes


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the dispatchers, restated (the library's own predicates are the authority)
def red_rows(M):
    r = max(cdiv(M, 1024), 16)
    return cdiv(r, 16) * 16


def nparts(M):
    return cdiv(M, red_rows(M))


def lanes(dt, C):
    """(vc, rl): channel-vector lanes and row lanes of a 256-thread reduction workgroup."""
    vc = C // VEC[dt]
    return vc, 256 // vc


def bnfin_ok(rows, C):
    return 0 < rows <= 64 and C % 64 == 0


def bnfin_grid(M, C):
    nsl = C // 64
    return max(min(cdiv(M, 32), cdiv(1024, nsl)), 1) * nsl


def pool_rows(N, H, W, C):
    if H % 2 or W % 2 or C % 8 or C // 4 > 256 or 256 % (C // 4):
        return 0
    return cdiv(W * (C // 4), 256) * cdiv(H // 2, 8) * N


def wraps(nvec):
    return nvec > WRAP_VECS


def fixed(V, C):
    return (256 * V) % C == 0


def rp_loops(rows):
    """Which loops of reduce_parts_1024<8> (128 part-lanes) run for lane 0."""
    return "8-deep" if rows > 896 else "2-deep" if rows > 128 else "tail"


# ---------------------------------------------------------------- case tables: (section, entry, dtype, shape, form)
STATS_C = {F32: (4, 8, 64, 96, 1024), BF16: (8, 40, 64, 96, 1024, 2048)}
STATS_M = (1, 15, 16, 17, 33, 1000)


def stats_form(dt, M, C):
    vc, rl = lanes(dt, C)
    last = M - (nparts(M) - 1) * red_rows(M)
    return f"col_stats<{dt}> vc={vc} rl={rl} red_rows={red_rows(M)}" + (" last=1" if last == 1 and nparts(M) > 1 else "")


def stats_cases():
    out = []
    for dt in (F32, BF16):
        for C in STATS_C[dt]:
            for M in STATS_M:
                out.append((dt, M, C))
        for C in ((64, 96) if dt == F32 else (40, 64)):
            out.append((dt, 16400, C))
    return out


FIN_ROWS = (1, 7, 128, 129, 300, 897, 1100)
FIN_C = (4, 12, 64, 100)
GEN_C = (8, 24, 96, 64, 512)
GEN_M = (2, 64, 1024, 1000)
WRAP_GEN = ((F32, 87383, 96), (F32, 16386, 512))          # smallest M with M * C / 4 > 2 097 152, plus one row
X3_C = (8, 96, 64, 2048)
C4_C = (4, 12, 36)
WRAP_X3 = ((174764, 96), (8194, 2048))                    # smallest M with M * C / 8 > 2 097 152, plus one row
FINAPP_ROWS = (1, 3, 4, 5, 64)
FINAPP_M = (1, 31, 33, 1056)
FINAPP_BIG = ((40000, 64), (1100, 2048))                  # 1250 strips of 32 pixels > 1024: the loop wraps;  nsl = 32
BWDX3 = (            # (M, C, given rows, route)
    (64, 128, 0, "fin"), (1040, 128, 0, "finalize+apply"), (64, 96, 0, "finalize+apply"), (64, 128, 3, "fin"), (64, 128, 70, "finalize+apply"),
    (64, 2048, 0, "fin"), (1040, 2048, 0, "finalize+apply"),
)
MASKS = ("none", "out", "hi", "recompute")
POOL = ((1, 2, 2, 8), (2, 4, 2, 8), (1, 6, 10, 64), (2, 10, 6, 64), (1, 16, 16, 64), (3, 8, 12, 96), (1, 8, 8, 12), (1, 4, 4, 1024))
AVG = ((1, 1, 4), (3, 49, 132), (2, 7, 512), (64, 16, 2048))
RATIOS = (0, 8, 64)


def pool_forms(shape):
    N, H, W, C = shape
    f = ["maxpool_fwd<f32>", "maxpool_bwd<f32>", "bn_bwd<f32>+pool_idx"]
    if C % 8 == 0:
        f += ["maxpool_fwd<bf16>", "maxpool_bwd<bf16>", "bn_bwd<bf16>+pool_idx", "maxpool_fwd_x3", "maxpool_fwd_x3+ywin", "maxpool_fwd_x3+ywin,out=NULL",
              "pool_win_bn_reduce+pool_bwd_bn_apply_x3"]
        f.append("pool_bwd_bn_reduce<8,false>+pool_bwd_bn_apply_x3" if pool_rows(N, H, W, C) else "nparts=0: maxpool_bwd+bn_bwd_x3(recompute)")
    else:
        f.append("maxpool_fwd<f32>+planes")
    geo = []
    if W == 2:
        geo.append("W=2")
    if H == 2:
        geo.append("H=2")
    if H // 2 < 4:
        geo.append("Ho<PFX_ROWS")
    elif (H // 2) % 4:
        geo.append("Ho%PFX_ROWS")
    if C // 4 == 256:
        geo.append("C/4=256")
    return f, geo


def all_cases():
    """Every launch shape of the file as (section, entry, dtype, shape, form)."""
    t = []
    for dt, M, C in stats_cases():
        t.append((1, "ab_col_stats", dt, (M, C), stats_form(dt, M, C)))
        t.append((1, "ab_col_sum", dt, (M, C), "colsum_finalize rows=%d" % nparts(M)))
        if dt == BF16:
            t.append((1, "ab_col_sum_x3", "x3", (M, C), "col_stats_x3 vc=%d rl=%d" % lanes(BF16, C)))
    for rows in FIN_ROWS:
        for C in FIN_C:
            t.append((2, "ab_bn_finalize", F32, (rows, C), f"bn_finalize<8> {rp_loops(rows)}" + ("" if C % 8 == 0 else " c<C")))
            t.append((2, "ab_bn_bwd_apply", F32, (rows, C), f"bn_bwd_finalize<8> {rp_loops(rows)}" + ("" if C % 8 == 0 else " c<C")))
    for dt in (F32, BF16):
        for C in GEN_C:
            for M in GEN_M:
                fx = "fixed" if fixed(VEC[dt], C) else "per-iteration"
                t.append((3, "ab_bn_apply", dt, (M, C), f"bn_apply<{dt}> {fx}"))
                t.append((3, "ab_bn_bwd", dt, (M, C), f"bn_bwd_reduce<{dt}> vc={lanes(dt, C)[0]} + bn_bwd_apply<{dt}> {fx}"))
    t.append((3, "ab_bn_bwd", F32, (64, 2048), "bn_bwd_reduce<f32> ysl=2"))
    for dt, M, C in WRAP_GEN:
        fx = "fixed" if fixed(VEC[dt], C) else "per-iteration"
        t.append((3, "ab_bn_apply", dt, (M, C), f"bn_apply<{dt}> {fx} wrap"))
        t.append((3, "ab_bn_bwd", dt, (M, C), f"bn_bwd_apply<{dt}> {fx} wrap"))
    for C in X3_C:
        fx = "fixed" if fixed(8, C) else "per-iteration"
        for e, k in (("ab_bn_apply_x3", "bn_apply_x3<false>"), ("ab_bn_apply_x3_resbn", "bn_apply_x3<true>"), ("ab_bn_apply_x3_respl", "bn_apply_x3<false,true>")):
            t.append((4, e, "x3", (66, C), f"{k} {fx}"))
    for C in C4_C:
        for e, k in (("ab_bn_apply_x3", "bn_apply_x3_c4 res=none"), ("ab_bn_apply_x3(res)", "bn_apply_x3_c4 res=f32"), ("ab_bn_apply_x3_respl", "bn_apply_x3_c4 res=planes")):
            t.append((4, e, "x3", (66, C), k))
    for M, C in WRAP_X3:
        fx = "fixed" if fixed(8, C) else "per-iteration"
        for e, k in (("ab_bn_apply_x3", "bn_apply_x3<false>"), ("ab_bn_apply_x3_resbn", "bn_apply_x3<true>"), ("ab_bn_apply_x3_respl", "bn_apply_x3<false,true>")):
            t.append((4, e, "x3", (M, C), f"{k} {fx} wrap"))
        t.append((4, "ab_bn_bwd_x3", "x3", (M, C), f"bn_bwd_apply_x3 {fx} wrap"))
    for rows in FINAPP_ROWS:
        for M in FINAPP_M:
            t.append((4, "ab_bn_fin_apply_x3", "x3", (rows, M, 64), "bn_fin_apply_x3<0,1,2> rows%%4=%d M%%32=%d" % (rows % 4, M % 32)))
    t.append((4, "ab_bn_fin_apply_x3", "x3", (5, 40000, 64), "bn_fin_apply_x3<0,1,2> strip wrap"))
    t.append((4, "ab_bn_fin_apply_x3", "x3", (5, 1100, 2048), "bn_fin_apply_x3<0,1,2> nsl=32"))
    for M, C, given, rt in BWDX3:
        for mk in MASKS:
            t.append((4, "ab_bn_bwd_x3", "x3", (M, C, given, mk), ("bn_fin_bwd_apply_x3" if rt == "fin" else "bn_bwd_finalize<8>+bn_bwd_apply_x3") +
                      f" mask={mk}" + (" given" if given else "") + (" ysl=2" if C == 2048 and not given else "")))
    for shape in POOL:
        f, geo = pool_forms(shape)
        for name in f:
            t.append((5, name.split("+")[0], "pool", shape + (name,), name + (" " + " ".join(geo) if geo else "")))
    for shape in AVG:
        for dt in (F32, BF16):
            if shape[2] % VEC[dt] == 0:
                t.append((6, "ab_avgpool_fwd", dt, shape, f"avgpool_fwd<{dt}>" + (" HW=1" if shape[1] == 1 else "") + (" ragged" if shape[2] % (32 * VEC[dt]) else "")))
    return t


# ---------------------------------------------------------------- operands
def _gen(*key):
    return torch.Generator().manual_seed(sum((int(v) + 7) * 131 ** i for i, v in enumerate(key)) % (1 << 31))


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def exact_problem(M, C, seed=0, balanced=True):
    """The exact-class operands of one BatchNorm over [M, C], all float64 (see the docstring)."""
    g = _gen(M, C, seed)
    o = types.SimpleNamespace(M=M, C=C)
    o.mu = _ints(g, -3, 3, (C,))
    o.sigma = 2.0 ** _ints(g, -1, 1, (C,))
    if balanced:
        assert M % 2 == 0, "balanced signs need an even M"
        base = torch.cat([torch.ones(M // 2, C), -torch.ones(M // 2, C)]).double()
        o.s = base.gather(0, torch.rand((M, C), generator=g).argsort(0))
    else:
        o.s = _ints(g, 0, 1, (M, C)) * 2 - 1
    o.y = o.mu + o.sigma * o.s
    o.gamma = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=g)]
    o.beta = _ints(g, -3, 2, (C,)) + 0.5
    o.res = _ints(g, -3, 3, (M, C))
    o.dout = _ints(g, -3, 3, (M, C))
    # a second BatchNorm for the BatchNorm-ed residual: integer beta, so the sum stays an odd multiple of 1/2
    o.mu2, o.sigma2 = _ints(g, -3, 3, (C,)), 2.0 ** _ints(g, -1, 1, (C,))
    o.res_y = o.mu2 + o.sigma2 * (_ints(g, 0, 1, (M, C)) * 2 - 1)
    o.gamma2 = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=g)]
    o.beta2 = _ints(g, -3, 3, (C,))
    o.bnp = hand_bnp(o.mu, o.sigma, o.gamma, o.beta)
    o.bnp2 = hand_bnp(o.mu2, o.sigma2, o.gamma2, o.beta2)
    return o


def hand_bnp(mu, sigma, gamma, beta):
    """bnp [4, C] = (scale, shift, mean, invstd) of a BatchNorm with batch mean mu, batch variance sigma^2, eps = 0."""
    invstd = 1.0 / sigma
    scale = gamma * invstd
    return torch.stack([scale, beta - mu * scale, mu, invstd])


def assert_sum_conditions(y):
    """Per channel sum |y| and sum y^2 over the launch <= 2^22: every fp32 partial sum is then exact in any order."""
    y = y.reshape(-1, y.shape[-1])
    assert float(y.abs().sum(0).max()) <= LIM and float((y * y).sum(0).max()) <= LIM
    assert bool((y * 2 == (y * 2).round()).all())


def hand_part(rows, C, count, mu, sigma, seed=0, kind="fwd"):
    """part [rows, C, 2] of exact integers whose column sums are (count * mu, count * (mu^2 + sigma^2)): mean = mu and var = sigma^2
    exactly in float64 (count a multiple of 4).  kind 'bwd': free integer sums (sum dz, sum dz * xhat)."""
    g = _gen(rows, C, count, seed)
    part = _ints(g, -4, 4, (rows, C, 2))
    if kind == "fwd":
        tot = torch.stack([count * mu, count * (mu * mu + sigma * sigma)], -1)
        assert bool((tot == tot.round()).all())
        part[-1] = tot - part[:-1].sum(0)
    return part


# ---------------------------------------------------------------- the reference, from the definitions (float64)
def ref_bnp(y, gamma, beta, eps):
    y = y.reshape(-1, y.shape[-1])
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    return torch.stack([scale, beta - mean * scale, mean, invstd]), var


def ref_running(rm, rv, mean, var, count, momentum):
    unb = var * count / (count - 1) if count > 1 else var
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unb


def ref_apply(y, bnp, relu, res=None, res_bnp=None):
    v = y * bnp[0] + bnp[1]
    if res is not None:
        v = v + (res * res_bnp[0] + res_bnp[1] if res_bnp is not None else res)
    return v.clamp_min(0.0) if relu else v


def ref_bwd(dout, y, bnp, mask, sums=None, keep_k2=True):
    """(dz, dbeta, dgamma, dy).  sums: (sum dz, sum dz * xhat) given from outside (a hand-built `part`).  keep_k2=False omits the
    xhat * k2 term: the planted error of the host file."""
    M = y.reshape(-1, y.shape[-1]).shape[0]
    dz = dout if mask is None else torch.where(mask > 0, dout, torch.zeros_like(dout))
    xhat = (y - bnp[2]) * bnp[3]
    red = tuple(range(y.dim() - 1))
    db, dg = (dz.sum(red), (dz * xhat).sum(red)) if sums is None else sums
    dy = bnp[0] * (dz - db / M - (xhat * dg / M if keep_k2 else 0.0))
    return dz, db, dg, dy


def scan_pool(a, last=False):
    """3x3 / 2 / pad 1 max-pool of a [N, H, W, C], written out: taps in scan order, a later tap wins only if strictly greater
    (last=True: greater or equal -- the LAST maximum, the planted error of the host file).  -> (pooled, winner code, flat input index)."""
    N, H, W, C = a.shape
    Ho, Wo = H // 2, W // 2
    pad = F.pad(a.permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf"))
    best = torch.full((N, C, Ho, Wo), float("-inf"), dtype=a.dtype)
    code = torch.zeros((N, C, Ho, Wo), dtype=torch.long)
    for dh in range(3):
        for dw in range(3):
            v = pad[:, :, dh:dh + 2 * Ho:2, dw:dw + 2 * Wo:2]
            win = (v >= best) if last else (v > best)
            win &= v > float("-inf")
            best = torch.where(win, v, best)
            code = torch.where(win, torch.full_like(code, dh * 3 + dw), code)
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    flat = (2 * ho - 1 + code // 3) * W + (2 * wo - 1 + code % 3)
    return best.permute(0, 2, 3, 1).contiguous(), code.permute(0, 2, 3, 1).contiguous(), flat


def ref_pool(a):
    """(pooled, winner code, flat input index [N, C, Ho, Wo]) from F.max_pool2d in float64; asserts torch chose the first maximum."""
    N, H, W, C = a.shape
    p, ind = F.max_pool2d(a.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    ho = torch.arange(H // 2).view(1, 1, -1, 1)
    wo = torch.arange(W // 2).view(1, 1, 1, -1)
    code = (ind // W - (2 * ho - 1)) * 3 + (ind % W - (2 * wo - 1))
    sp, scode, sflat = scan_pool(a)
    assert torch.equal(sp, p.permute(0, 2, 3, 1)) and torch.equal(sflat, ind), "torch's winner is not the first maximum in scan order"
    return sp, code.permute(0, 2, 3, 1).contiguous(), ind


def pool_gather(y, flat):
    """y [N, H, W, C] at the winners -> [N, Ho, Wo, C]."""
    N, H, W, C = y.shape
    return y.permute(0, 3, 1, 2).reshape(N, C, H * W).gather(2, flat.reshape(N, C, -1)).reshape(flat.shape).permute(0, 2, 3, 1).contiguous()


def pool_scatter(dpool, flat, H, W):
    """Max-pool backward: dpool [N, Ho, Wo, C] added at the winners -> [N, H, W, C]."""
    N, Ho, Wo, C = dpool.shape
    da = torch.zeros((N, C, H * W), dtype=dpool.dtype)
    da.scatter_add_(2, flat.reshape(N, C, -1), dpool.permute(0, 3, 1, 2).reshape(N, C, -1))
    return da.reshape(N, C, H, W).permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------- the bounds of the random class (float64, first order, see the docstring)
def chain(rows, rl):
    return cdiv(rows, rl) + rl


def stats_bound(x, rl, rows=None):
    """(e_S, e_Q) per channel for the column sums of x [M, C] reduced by workgroups of `rows` rows with rl row lanes."""
    M = x.shape[0]
    L = chain(min(rows or red_rows(M), M), rl)
    return L * U * x.abs().sum(0), (L + 1) * U * (x * x).sum(0)


def bnp_bound(y, gamma, beta, eps, eS, eQ):
    """Error bounds of (scale, shift, mean, invstd) [4, C] given those of the two column sums."""
    M = y.shape[0]
    bnp, var = ref_bnp(y, gamma, beta, eps)
    scale, shift, mean, invstd = bnp
    e_mean = eS / M
    e_var = eQ / M + 2 * mean.abs() * e_mean
    e_inv = 0.5 * invstd ** 3 * e_var + U * invstd
    e_scale = gamma.abs() * e_inv + U * scale.abs()
    e_shift = mean.abs() * e_scale + scale.abs() * (e_mean + U * mean.abs()) + U * (mean * scale).abs() + U * shift.abs()
    return torch.stack([e_scale, e_shift, e_mean + U * mean.abs(), e_inv])


def apply_bound(y, bnp, e_bnp, res=None):
    """Bound of y * scale + shift (+ res) evaluated in fp32 with parameters off by e_bnp (ReLU does not enlarge it)."""
    v = (y * bnp[0]).abs() + bnp[1].abs()
    b = y.abs() * e_bnp[0] + e_bnp[1] + 2 * U * v
    if res is not None:
        b = b + U * (v + res.abs())
    return b


def bwd_bound(dout, y, bnp, mask, rl, rows, pre=None, gathered=0, exact_sums=False):
    """Bounds (e_dbeta, e_dgamma, e_dy) of the BatchNorm backward on fp32 inputs, the reference reading the SAME fp32 bnp.
    pre: the pre-activation when the kernel recomputes the mask from it -- an element within 4 u (|y scale| + |shift|) of 0 may take either
    value.  gathered: roundings a gathered dout carries (the pooled gradient summed over up to 4 windows).  exact_sums: the two column sums
    are known to be exact (the exact class, where they are asserted bit-equal): only the elementwise arithmetic of dy is left."""
    M = y.shape[0]
    dz, db, dg, dy = ref_bwd(dout, y, bnp, mask)
    xhat = (y - bnp[2]) * bnp[3]
    amb = torch.zeros_like(dout)
    if pre is not None:
        amb = (pre.abs() <= 4 * U * ((y * bnp[0]).abs() + bnp[1].abs())).double() * dout.abs()
    L = chain(min(rows, M), rl)
    e_db = (L + gathered) * U * dz.abs().sum(0) + amb.sum(0)
    e_dg = (L + 3 + gathered) * U * (dz * xhat).abs().sum(0) + (amb * xhat.abs()).sum(0)
    if exact_sums:
        e_db, e_dg = torch.zeros_like(e_db), torch.zeros_like(e_dg)
    e_k1, e_k2 = (e_db + 3 * U * db.abs()) / M, (e_dg + 3 * U * dg.abs()) / M
    e_dy = bnp[0].abs() * (e_k1 + xhat.abs() * e_k2 + (6 + gathered) * U * (dz.abs() + (db / M).abs() + (xhat * dg / M).abs()) + amb)
    return e_db, e_dg, e_dy


# ---------------------------------------------------------------- checkers
TALLY = {"exact": 0, "ratio": {}}


def _cpu64(t):
    return t.detach().cpu().double()


def assert_bits(what, got, ref):
    """got (any dtype, any device) == ref (float64), entry by entry."""
    g = _cpu64(got).reshape(ref.shape)
    bad = g != ref
    n = int(bad.sum())
    assert n == 0, f"{what}: {n} of {ref.numel()} entries differ, first at {tuple(int(v) for v in bad.nonzero()[0])}: got {float(g[bad][0])!r}, expected {float(ref[bad][0])!r}"
    TALLY["exact"] += 1


def assert_ulp(what, got, ref, ulps=1):
    g = _cpu64(got).reshape(ref.shape)
    err = (g - ref).abs()
    lim = ulps * 2.0 ** -23 * ref.abs()
    assert bool((err <= lim).all()), f"{what}: off by {float((err / lim.clamp_min(1e-300)).max()):.2f} x the {ulps} ulp allowed"


def assert_bound(what, got, ref, bound, section=None):
    """|got - ref| <= MARGIN * bound entry by entry (a zero bound demands equality); prints and tallies err / bound."""
    g = _cpu64(got).reshape(ref.shape)
    err = (g - ref).abs()
    bound = bound.expand_as(ref) if bound.shape != ref.shape else bound
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    r = float(ratio.max()) if ratio.numel() else 0.0
    print(f"err/bound {r:8.4f}  {what}")
    if section is not None and r > TALLY["ratio"].get(section, (-1.0, ""))[0]:
        TALLY["ratio"][section] = (r, what)
    assert r <= MARGIN, f"{what}: error {r:.3f} x its first-order bound (allowed {MARGIN})"
    return r


def assert_planes(what, planes, ref):
    """Split planes [2, ...] on the device == K.split of the float64 result rounded to fp32 (as values: like assert_bits, the sign of a
    zero is not compared -- float64 and the kernels order the subtractions of dy differently; an unwritten NaN differs from everything)."""
    from artiboost_amd import kernels as K
    exp = K.split(ref.float().cuda())
    bad = (planes.float() != exp.float().reshape(planes.shape))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} plane entries differ"
    TALLY["exact"] += 1


def assert_running_once(what, rm, rv, rm0, rv0, mean, var, count, momentum):
    """The running statistics equal ONE update from (rm0, rv0): running_mean exactly, running_var within 1 ulp of fp32."""
    erm, erv = ref_running(rm0, rv0, mean, var, count, momentum)
    assert_bits(what + " running_mean", rm, erm)
    assert_ulp(what + " running_var", rv, erv, 1)


# ---------------------------------------------------------------- device plumbing
def dev(t, dt=F32):
    """float64 CPU -> device tensor of the dtype; the value must survive the conversion (the exact class is representable)."""
    d = t.to(TD[dt])
    assert torch.equal(d.double(), t), "an operand of the exact class is not representable"
    return d.cuda().contiguous()


def rdev(t):
    return t.float().cuda().contiguous()


def nan(*shape, dtype=torch.float32):
    if dtype == torch.uint8:
        return torch.full(shape, 0xEE, dtype=dtype, device="cuda")
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def abi(fn, *args):
    """The C ABI through the package's own loader; returns the return code (the dispatcher binding raises on a non-zero code and names
    it in the message; the ctypes binding returns it)."""
    from artiboost_amd import _lib as L
    try:
        return getattr(L.lib(), fn)(*args, L.stream())
    except RuntimeError as e:
        m = re.search(r"failed with code (-?\d+)", str(e))
        if m is None:
            raise
        return int(m.group(1))


def call(fn, *args):
    rc = abi(fn, *args)
    assert rc == 0, f"{fn} returned {rc}"


def DTC(dt):
    return 0 if dt == F32 else 1


def twice(launch):
    """Runs an exact launch twice into fresh NaN-filled outputs; the second result must be bit-equal to the first."""
    a = launch()
    b = launch()
    torch.cuda.synchronize()
    for x, z in zip(a, b):
        if x is not None:
            assert torch.equal(x.view(torch.uint8), z.view(torch.uint8)), "a second call differs from the first"
    return a


def rounded(ref, dt):
    """The float64 result as the kernel stores it: exact in fp32 (asserted), then rounded to nearest even for bf16."""
    f = ref.float()
    return f.double() if dt == F32 else f.bfloat16().double()


# ---------------------------------------------------------------- 1. statistics
def _block_sums(x, M):
    """Per-workgroup (sum, sum of squares) [nparts, C, 2] of x [M, C] in float64, the partition restated from red_rows."""
    r = red_rows(M)
    rows = []
    for b in range(nparts(M)):
        blk = x[b * r:min((b + 1) * r, M)]
        rows.append(torch.stack([blk.sum(0), (blk * blk).sum(0)], -1))
    return torch.stack(rows)


@pytest.mark.parametrize("dt,M,C", stats_cases(), ids=lambda v: str(v))
def test_column_statistics_exact(dt, M, C):
    """ab_col_stats, ab_col_sum and (bf16) ab_col_sum_x3: the row count, every partial row against the float64 sums of its own rows, the
    column totals -- bit for bit on the exact class."""
    from artiboost_amd import _lib as L
    o = exact_problem(M, C, 1, balanced=False)
    assert_sum_conditions(o.y)
    rows = nparts(M)
    assert L.lib().ab_col_stats_nparts(M) == rows
    x = dev(o.y, dt)
    ref = _block_sums(o.y, M)

    def stats():
        part = nan(rows, C, 2)
        call("ab_col_stats", x, DTC(dt), M, C, part)
        return (part,)

    (part,) = twice(stats)
    assert_bits(f"col_stats<{dt}> {(M, C)} partial rows", part, ref)

    def colsum():
        part, out = nan(rows, C, 2), nan(C)
        call("ab_col_sum", x, DTC(dt), M, C, part, out)
        return part, out

    part, tot = twice(colsum)
    assert_bits(f"col_sum<{dt}> {(M, C)} rows", part, ref)
    assert_bits(f"col_sum<{dt}> {(M, C)} totals", tot, o.y.sum(0).float().double())
    if dt == BF16:
        # a split tensor with a non-zero lo plane: y + 2^-9 t, t in {-1, 0, 1}: hi = y, lo = t 2^-9
        t = _ints(_gen(M, C, 5), -1, 1, (M, C)) * 2.0 ** -9
        v = o.y + t
        hi, lo = dev(o.y, BF16), dev(t, BF16)

        def colsum3():
            part, out = nan(rows, C, 2), nan(C)
            call("ab_col_sum_x3", hi, lo, M, C, part, out)
            return part, out

        part, tot = twice(colsum3)
        assert_bits(f"col_sum_x3 {(M, C)} rows", part[..., 0], _block_sums(v, M)[..., 0])
        assert_bits(f"col_sum_x3 {(M, C)} totals", tot, v.sum(0).float().double())          # exact in double, rounded once


def test_column_statistics_refusals():
    """AB_ESHAPE: more than 256 channel vectors, and C not a multiple of the vector width.  Nothing is written."""
    for fn, dt, C in (("ab_col_stats", F32, 1028), ("ab_col_stats", BF16, 2056), ("ab_col_stats", F32, 6), ("ab_col_stats", BF16, 12),
                      ("ab_col_sum", F32, 1028), ("ab_col_sum", BF16, 2056), ("ab_col_sum", BF16, 12)):
        x = torch.zeros((16, C), dtype=TD[dt], device="cuda")
        part, out = nan(1, C, 2), nan(C)
        rc = abi(fn, x, DTC(dt), 16, C, part) if fn == "ab_col_stats" else abi(fn, x, DTC(dt), 16, C, part, out)
        assert rc == ESHAPE, (fn, dt, C, rc)
        torch.cuda.synchronize()
        assert bool(torch.isnan(part).all()) and bool(torch.isnan(out).all())
    for C in (2056, 12):
        z = torch.zeros((16, C), dtype=torch.bfloat16, device="cuda")
        assert abi("ab_col_sum_x3", z, z, 16, C, nan(1, C, 2), nan(C)) == ESHAPE


# ---------------------------------------------------------------- 2. finalize
def _fin_problem(rows, C, count, seed=0):
    g = _gen(rows, C, count, seed, 2)
    mu, sigma = _ints(g, -3, 3, (C,)), 2.0 ** _ints(g, -1, 1, (C,))
    gamma = torch.tensor([-2.0, -1.0, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 4, (C,), generator=g)]
    beta = _ints(g, -3, 2, (C,)) + 0.5
    rm0, rv0 = _ints(g, -8, 8, (C,)) / 4, _ints(g, 1, 16, (C,)) / 4
    return types.SimpleNamespace(mu=mu, sigma=sigma, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, part=hand_part(rows, C, count, mu, sigma, seed),
                                 bnp=hand_bnp(mu, sigma, gamma, beta), count=count)


@pytest.mark.parametrize("C", FIN_C)
@pytest.mark.parametrize("rows", FIN_ROWS)
def test_bn_finalize_hand_built_rows(rows, C):
    """ab_bn_finalize on hand-built integer rows (all three loops of reduce_parts_1024, the c < C guard): bnp bit-equal to float64, the
    running statistics one update; running statistics absent; momentum 1/2 and 1/4."""
    for momentum, count in ((0.5, 4 * rows), (0.25, 64)):
        p = _fin_problem(rows, C, count, int(momentum * 4))
        part, gamma, beta = dev(p.part), dev(p.gamma), dev(p.beta)

        def fin(with_running=True):
            bnp = nan(4, C)
            rm, rv = (dev(p.rm0), dev(p.rv0)) if with_running else (None, None)
            call("ab_bn_finalize", part, rows, C, count, gamma, beta, 0.0, momentum, rm, rv, bnp)
            return bnp, rm, rv

        bnp, rm, rv = twice(fin)
        assert_bits(f"bn_finalize rows={rows} C={C} bnp", bnp, p.bnp)
        assert_running_once(f"bn_finalize rows={rows} C={C}", rm, rv, p.rm0, p.rv0, p.mu, p.sigma ** 2, count, momentum)
        bnp, _, _ = fin(False)
        assert_bits(f"bn_finalize rows={rows} C={C} bnp, no running statistics", bnp, p.bnp)


@pytest.mark.parametrize("C", (4, 100))
def test_bn_finalize_count_one_and_the_variance_clamp(C):
    """count = 1: the unbiased variance is the biased one (no division by count - 1 = 0).  A row pair whose q / count - mean^2 is
    negative in float64: the variance is clamped to 0, invstd = 1 / sqrt(eps) with eps = 2^-10, i.e. exactly 32."""
    g = _gen(C, 9)
    mu, sigma = _ints(g, -3, 3, (C,)), 2.0 ** _ints(g, -1, 1, (C,))
    gamma, beta = torch.ones(C, dtype=torch.float64), _ints(g, -3, 2, (C,)) + 0.5
    rm0, rv0 = _ints(g, -8, 8, (C,)) / 4, _ints(g, 1, 16, (C,)) / 4
    part = torch.stack([mu, mu * mu + sigma * sigma], -1).unsqueeze(0)
    bnp, rm, rv = nan(4, C), dev(rm0), dev(rv0)
    call("ab_bn_finalize", dev(part), 1, C, 1, dev(gamma), dev(beta), 0.0, 0.5, rm, rv, bnp)
    assert_bits("bn_finalize count=1 bnp", bnp, hand_bnp(mu, sigma, gamma, beta))
    assert_running_once("bn_finalize count=1", rm, rv, rm0, rv0, mu, sigma ** 2, 1, 0.5)
    # mean = 3, q / count = 8 < 9
    rows, count, eps = 7, 28, 2.0 ** -10
    part = torch.zeros((rows, C, 2), dtype=torch.float64)
    part[:, :, 0], part[:, :, 1] = 12.0, 32.0
    ref_var = part[:, :, 1].sum(0) / count - (part[:, :, 0].sum(0) / count) ** 2
    assert float(ref_var.max()) < 0
    bnp, rm, rv = nan(4, C), dev(rm0), dev(rv0)
    call("ab_bn_finalize", dev(part), rows, C, count, dev(gamma), dev(beta), eps, 0.5, rm, rv, bnp)
    three = torch.full((C,), 3.0, dtype=torch.float64)
    assert_bits("bn_finalize clamp bnp", bnp, torch.stack([gamma * 32, beta - 3 * gamma * 32, three, three * 0 + 32]))
    assert_running_once("bn_finalize clamp", rm, rv, rm0, rv0, three, three * 0, count, 0.5)


@pytest.mark.parametrize("C", FIN_C)
@pytest.mark.parametrize("rows", FIN_ROWS)
def test_bn_backward_finalize_hand_built_rows(rows, C):
    """ab_bn_bwd_apply with a given `part`: dgamma, dbeta and bwdp are the float64 column sums of the rows, and dy uses them (M = 2)."""
    M = 2
    o = exact_problem(M, C, 3)
    part = hand_part(rows, C, 0, None, None, 1, kind="bwd")
    sums = (part[:, :, 0].sum(0), part[:, :, 1].sum(0))
    dz, _, _, dy = ref_bwd(o.dout, o.y, o.bnp, None, sums=sums)
    d = types.SimpleNamespace(dout=dev(o.dout), y=dev(o.y), bnp=dev(o.bnp), part=dev(part))

    def run():
        bwdp, dg, db, dyo = nan(2, C), nan(C), nan(C), nan(M, C)
        call("ab_bn_bwd_apply", d.dout, None, d.y, d.bnp, 0, M, C, 0, d.part, rows, bwdp, dg, db, dyo, None)
        return bwdp, dg, db, dyo

    bwdp, dg, db, dyo = twice(run)
    assert_bits(f"bn_bwd_finalize rows={rows} C={C} dbeta", db, sums[0])
    assert_bits(f"bn_bwd_finalize rows={rows} C={C} dgamma", dg, sums[1])
    assert_bits(f"bn_bwd_finalize rows={rows} C={C} bwdp", bwdp, torch.stack(sums))
    assert_bits(f"bn_bwd_finalize rows={rows} C={C} dy", dyo, dy)


# ---------------------------------------------------------------- 3. apply and backward, generic dtypes
def _mask_of(o, relu, with_res):
    """(float64 mask or None, the stored activation) for relu 0 / 1 (mask from `out`) / 2 (recomputed from y: no residual)."""
    if relu == 0:
        return None, None
    act = ref_apply(o.y, o.bnp, True, o.res if (with_res and relu == 1) else None)
    return (act > 0).double(), act


def _generic_case(dt, M, C, seed=0, combos=None):
    o = exact_problem(M, C, seed, balanced=(M % 2 == 0 and M <= 4096))
    assert_sum_conditions(o.y)
    pow2 = (M & (M - 1)) == 0
    y, res, dout, bnp = dev(o.y, dt), dev(o.res, dt), dev(o.dout, dt), dev(o.bnp)
    vc, rl = lanes(dt, min(C, 256 * VEC[dt]))
    what = f"<{dt}> {(M, C)}"
    for relu, with_res in combos or ((0, False), (0, True), (1, False), (1, True)):
        ref = ref_apply(o.y, o.bnp, relu, o.res if with_res else None)

        def app():
            out = nan(M, C, dtype=TD[dt])
            call("ab_bn_apply", y, res if with_res else None, bnp, DTC(dt), M, C, relu, out)
            return (out,)

        (out,) = twice(app)
        assert_bits(f"bn_apply{what} relu={relu} res={with_res}", out, rounded(ref, dt))
    bwd_combos = [(r, w, True) for r, w in combos] if combos else ((0, False, False), (1, True, True), (1, False, False), (2, False, True), (2, False, False))
    for relu, with_res, want_dz in bwd_combos:
        mask, act = _mask_of(o, relu, with_res)
        dz, db, dg, dy = ref_bwd(o.dout, o.y, o.bnp, mask)
        actd = dev(act, dt) if relu == 1 else None

        def bwd():
            part, bwdp, dgo, dbo = nan(nparts(M), C, 2), nan(2, C), nan(C), nan(C)
            dyo, dzo = nan(M, C, dtype=TD[dt]), (nan(M, C, dtype=TD[dt]) if want_dz else None)
            call("ab_bn_bwd", dout, actd, y, bnp, DTC(dt), M, C, relu, part, bwdp, dgo, dbo, dyo, dzo)
            return part, bwdp, dgo, dbo, dyo, dzo

        part, bwdp, dgo, dbo, dyo, dzo = twice(bwd)
        w = f"bn_bwd{what} relu={relu} res={with_res}"
        assert_bits(w + " dbeta", dbo, db)
        assert_bits(w + " dgamma", dgo, dg)
        assert_bits(w + " bwdp", bwdp, torch.stack([db, dg]))
        assert_bits(w + " partial rows", part.double().sum(0), torch.stack([db, dg], -1))
        if want_dz:
            assert_bits(w + " dz", dzo, dz)
        if pow2:
            assert_bits(w + " dy", dyo, rounded(dy, dt))
        else:
            _, _, e_dy = bwd_bound(o.dout, o.y, o.bnp, mask, rl, red_rows(M), exact_sums=True)
            if dt == BF16:
                e_dy = e_dy + 2.0 ** -8 * dy.abs()          # the store rounds to 8 significant bits: half an ulp is 2^-8 relative
            assert_bound(w + " dy", dyo, dy, e_dy, 3)


@pytest.mark.parametrize("M", GEN_M)
@pytest.mark.parametrize("C", GEN_C)
@pytest.mark.parametrize("dt", (F32, BF16))
def test_bn_apply_and_backward_generic_exact(dt, C, M):
    """ab_bn_apply and ab_bn_bwd in both dtypes, relu 0 / 1 / 2, residual and dz_out on and off: out, dz, dgamma, dbeta, bwdp and the
    partial-row sums bit-equal to float64; dy bit-equal where M is a power of two and within the derived bound at M = 1000."""
    _generic_case(dt, M, C)


def test_bn_backward_2048_channels_in_two_slices():
    """C = 2048 in fp32 is 512 channel vectors: bn_bwd_reduce_kernel runs with gridDim.y = 2."""
    _generic_case(F32, 64, 2048, combos=((1, True), (2, False)))


@pytest.mark.parametrize("dt,M,C", WRAP_GEN, ids=lambda v: str(v))
def test_bn_apply_and_backward_generic_grid_wrap(dt, M, C):
    """More than 8192 x 256 vectors: the grid-stride loops wrap, with the channel parameters loaded once (C = 512) or per iteration
    (C = 96), and the last iteration is partial."""
    assert wraps(M * C // VEC[dt]) and not wraps((M - 2) * C // VEC[dt])
    _generic_case(dt, M, C, combos=((1, True),))


def _random_problem(M, C, ratio, seed):
    """randn operands with a per-channel scale in [1/2, 2] and a per-channel offset of `ratio` standard deviations, rounded to fp32."""
    g = _gen(M, C, ratio, seed, 77)
    sd = 0.5 + 1.5 * torch.rand(C, generator=g, dtype=torch.float64)
    off = sd * ratio * (torch.randint(0, 2, (C,), generator=g).double() * 2 - 1)
    o = types.SimpleNamespace(M=M, C=C)
    f32 = lambda t: t.float().double()          # noqa: E731
    o.y = f32(torch.randn((M, C), generator=g, dtype=torch.float64) * sd + off)
    o.gamma = f32(0.5 + torch.rand(C, generator=g, dtype=torch.float64)) * (torch.randint(0, 2, (C,), generator=g).double() * 2 - 1)
    o.beta = f32(torch.randn(C, generator=g, dtype=torch.float64))
    o.res = f32(torch.randn((M, C), generator=g, dtype=torch.float64))
    o.dout = f32(torch.randn((M, C), generator=g, dtype=torch.float64))
    return o


def _random_forward(o, eps=1e-5, section=3):
    """col_stats -> bn_finalize -> bn_apply on fp32 randn operands, each stage against float64 within its derived bound.  Returns the
    kernel's bnp (device) and the observed relative error of invstd."""
    M, C = o.M, o.C
    vc, rl = lanes(F32, C)
    y, what = rdev(o.y), f"random {(M, C)}"
    part, bnp, out = nan(nparts(M), C, 2), nan(4, C), nan(M, C)
    call("ab_col_stats", y, 0, M, C, part)
    call("ab_bn_finalize", part, nparts(M), C, M, rdev(o.gamma), rdev(o.beta), eps, 0.1, None, None, bnp)
    call("ab_bn_apply", y, rdev(o.res), bnp, 0, M, C, 1, out)
    eS, eQ = stats_bound(o.y, rl)
    tot = _cpu64(part).sum(0)
    assert_bound(what + " sum x", tot[:, 0], o.y.sum(0), eS, section)
    assert_bound(what + " sum x^2", tot[:, 1], (o.y * o.y).sum(0), eQ, section)
    ref, _ = ref_bnp(o.y, o.gamma, o.beta, eps)
    e_bnp = bnp_bound(o.y, o.gamma, o.beta, eps, eS, eQ)
    for k, name in enumerate(("scale", "shift", "mean", "invstd")):
        assert_bound(f"{what} {name}", bnp[k], ref[k], e_bnp[k], section)
    assert_bound(what + " out", out, ref_apply(o.y, ref, True, o.res), apply_bound(o.y, ref, e_bnp, o.res), section)
    return bnp, float(((_cpu64(bnp[3]) - ref[3]).abs() / ref[3]).max()), float((e_bnp[3] / ref[3]).max())


def _random_backward(o, bnp, section=3):
    """ab_bn_bwd on the kernel's own fp32 bnp; the float64 reference reads the same fp32 values."""
    M, C = o.M, o.C
    vc, rl = lanes(F32, C)
    b64 = _cpu64(bnp)
    y, dout = rdev(o.y), rdev(o.dout)
    for relu in (0, 1, 2):
        pre = o.y * b64[0] + b64[1]
        act = (pre + (o.res if relu == 1 else 0)).clamp_min(0).float().double()
        mask = None if relu == 0 else (act > 0).double() if relu == 1 else (pre > 0).double()
        dz, db, dg, dy = ref_bwd(o.dout, o.y, b64, mask)
        part, bwdp, dgo, dbo, dyo, dzo = nan(nparts(M), C, 2), nan(2, C), nan(C), nan(C), nan(M, C), nan(M, C)
        call("ab_bn_bwd", dout, rdev(act) if relu == 1 else None, y, bnp, 0, M, C, relu, part, bwdp, dgo, dbo, dyo, dzo)
        e_db, e_dg, e_dy = bwd_bound(o.dout, o.y, b64, mask, rl, red_rows(M), pre=pre if relu == 2 else None)
        w = f"random {(M, C)} relu={relu}"
        assert_bound(w + " dbeta", dbo, db, e_db, section)
        assert_bound(w + " dgamma", dgo, dg, e_dg, section)
        assert_bound(w + " dy", dyo, dy, e_dy, section)
        if relu != 2:
            assert_bits(w + " dz", dzo, dz)


@pytest.mark.parametrize("M,C", ((1000, 96), (1024, 64), (4099, 8), (600, 1024)))
def test_bn_forward_and_backward_random_class(M, C):
    """Statistics, finalize, apply and backward on randn operands (offset 2 standard deviations), each held to its derived bound."""
    o = _random_problem(M, C, 2, 0)
    bnp, _, _ = _random_forward(o)
    _random_backward(o, bnp)


OFFSET_REPORT = {}


@pytest.mark.parametrize("ratio", RATIOS)
def test_offset_to_spread_ratio(ratio):
    """|mean| / std in {0, 8, 64} at C = 64, M = 4096: the fp32 sum x, sum x^2 design loses the variance to cancellation as the ratio
    grows; the derived bound says by how much and the kernel is held to it.  Observed relative error of invstd (bound in brackets), on an
    MI355X: see the docstring of the file."""
    o = _random_problem(4096, 64, ratio, 1)
    bnp, rel, rel_bound = _random_forward(o, section="offset")
    OFFSET_REPORT[ratio] = (rel, rel_bound)
    print(f"offset ratio {ratio}: relative error of invstd {rel:.3e} (first-order bound {rel_bound:.3e})")
    _random_backward(o, bnp, section="offset")


# ---------------------------------------------------------------- 4. split-plane producers
def _x3_apply_variants(o, d, M, C, relu, want_out):
    """(name, reference, launch) of the three residual forms of bn_apply_x3 plus the plain one."""
    from artiboost_amd import kernels as K
    res_pl = K.split(d.res)

    def mk(fn, *args):
        def launch():
            out = nan(M, C) if want_out else None
            pl = nan(2, M, C, dtype=torch.bfloat16)
            rc = abi(fn, *args, M, C, relu, out, pl[0], pl[1])
            return rc, out, pl
        return launch
    yield "none", ref_apply(o.y, o.bnp, relu), mk("ab_bn_apply_x3", d.y, None, d.bnp)
    yield "f32", ref_apply(o.y, o.bnp, relu, o.res), mk("ab_bn_apply_x3", d.y, d.res, d.bnp)
    yield "planes", ref_apply(o.y, o.bnp, relu, o.res), mk("ab_bn_apply_x3_respl", d.y, res_pl[0], res_pl[1], d.bnp)
    yield "bn", ref_apply(o.y, o.bnp, relu, o.res_y, o.bnp2), mk("ab_bn_apply_x3_resbn", d.y, d.res_y, d.bnp, d.bnp2)


def _x3_dev(o):
    return types.SimpleNamespace(y=dev(o.y), res=dev(o.res), res_y=dev(o.res_y), dout=dev(o.dout), bnp=dev(o.bnp), bnp2=dev(o.bnp2))


def _x3_apply_case(M, C, combos):
    o = exact_problem(M, C, 4, balanced=False)
    d = _x3_dev(o)
    for relu, want_out in combos:
        for name, ref, launch in _x3_apply_variants(o, d, M, C, relu, want_out):
            rc, out, pl = launch()
            w = f"bn_apply_x3 {(M, C)} res={name} relu={relu} out={'f32' if want_out else 'NULL'}"
            if name == "bn" and C % 8:
                assert rc == ESHAPE, f"{w}: expected AB_ESHAPE, got {rc}"
                torch.cuda.synchronize()
                assert bool(torch.isnan(pl.float()).all())
                continue
            assert rc == 0, (w, rc)
            rc, out2, pl2 = launch()
            assert torch.equal(pl.view(torch.int16), pl2.view(torch.int16)), w + ": a second call differs"
            assert_planes(w, pl, ref)
            if want_out:
                assert_bits(w + " fp32", out, ref)


@pytest.mark.parametrize("C", X3_C + C4_C)
def test_bn_apply_x3_every_residual_form(C):
    """ab_bn_apply_x3 / _resbn / _respl: 8 channels per lane with fixed (C = 8, 64, 2048) and per-iteration (C = 96) parameters, and the
    4-channel kernel (C = 4, 12, 36) with no, an fp32 and a plane residual, which _resbn refuses; out NULL and given."""
    _x3_apply_case(66, C, ((1, True), (0, False), (1, False)))


@pytest.mark.parametrize("M,C", WRAP_X3, ids=lambda v: str(v))
def test_bn_apply_x3_and_backward_grid_wrap(M, C):
    """More than 8192 x 256 eight-channel vectors: bn_apply_x3_kernel in its three forms and bn_bwd_apply_x3_kernel wrap, per-iteration
    (C = 96) and fixed (C = 2048) parameters, last iteration partial."""
    assert wraps(M * C // 8) and not wraps((M - 2) * C // 8)
    _x3_apply_case(M, C, ((1, False),))
    rows = nparts(M)
    assert not bnfin_ok(rows, C)
    o = exact_problem(M, C, 4, balanced=False)
    mask = (ref_apply(o.y, o.bnp, True) > 0).double()
    dz, db, dg, dy = ref_bwd(o.dout, o.y, o.bnp, mask)
    y, dout, bnp = dev(o.y), dev(o.dout), dev(o.bnp)
    part, bwdp, dgo, dbo, pl = nan(rows, C, 2), nan(2, C), nan(C), nan(C), nan(2, M, C, dtype=torch.bfloat16)
    call("ab_bn_bwd_x3", dout, None, 0, y, bnp, M, C, 2, part, 0, bwdp, dgo, dbo, pl[0], pl[1], None)
    assert_bits(f"bn_bwd_x3 wrap {(M, C)} dbeta", dbo, db)
    assert_bits(f"bn_bwd_x3 wrap {(M, C)} dgamma", dgo, dg)
    vc, rl = lanes(F32, min(C, 1024))
    _, _, e_dy = bwd_bound(o.dout, o.y, o.bnp, mask, rl, red_rows(M), exact_sums=True)
    got = pl.float().double().sum(0)
    assert_bound(f"bn_bwd_x3 wrap {(M, C)} dy (hi + lo)", got, dy, e_dy + 2.0 ** -16 * dy.abs(), 4)


def _finapp_case(rows, M, C, seed=0):
    from artiboost_amd import kernels as K
    count, momentum = 4 * rows, 0.25
    p = _fin_problem(rows, C, count, seed)
    o = exact_problem(M, C, 6, balanced=False)
    # y around the BatchNorm of `p`: the statistics come from `part`, the pixels only have to keep the pre-activation off 0
    y = p.mu + p.sigma * o.s
    d = types.SimpleNamespace(y=dev(y), res=dev(o.res), res_y=dev(o.res_y), bnp2=dev(o.bnp2), part=dev(p.part), gamma=dev(p.gamma), beta=dev(p.beta))
    res_pl = K.split(d.res)
    assert bnfin_ok(rows, C) and bool(K.bn_fin_apply_x3_ok(d.part, C))
    sep = nan(4, C)
    call("ab_bn_finalize", d.part, rows, C, count, d.gamma, d.beta, 0.0, momentum, None, None, sep)
    for res_kind, relu, want_out in ((0, 1, True), (0, 0, False), ("f32", 1, False), (1, 1, True), (2, 1, False)):
        res = o.res if res_kind in ("f32", 1) else o.res_y if res_kind == 2 else None
        ref = ref_apply(y, p.bnp, relu, res, o.bnp2 if res_kind == 2 else None)

        def launch():
            bnp, rm, rv = nan(4, C), dev(p.rm0), dev(p.rv0)
            out, pl = (nan(M, C) if want_out else None), nan(2, M, C, dtype=torch.bfloat16)
            call("ab_bn_fin_apply_x3", d.part, rows, count, d.gamma, d.beta, 0.0, momentum, rm, rv, bnp, d.y,
                 d.res if res_kind == "f32" else d.res_y if res_kind == 2 else None, res_pl[0] if res_kind == 1 else None,
                 res_pl[1] if res_kind == 1 else None, d.bnp2 if res_kind == 2 else None, M, C, relu, out, pl[0], pl[1])
            return bnp, rm, rv, out, pl

        bnp, rm, rv, out, pl = twice(launch)
        w = f"bn_fin_apply_x3 rows={rows} {(M, C)} res={res_kind} relu={relu}"
        assert_bits(w + " bnp", bnp, p.bnp)
        assert torch.equal(bnp, sep), w + ": bnp differs from ab_bn_finalize on the same rows"
        assert_running_once(w, rm, rv, p.rm0, p.rv0, p.mu, p.sigma ** 2, count, momentum)
        assert_planes(w, pl, ref)
        if want_out:
            assert_bits(w + " fp32", out, ref)


@pytest.mark.parametrize("M", FINAPP_M)
@pytest.mark.parametrize("rows", FINAPP_ROWS)
def test_bn_fin_apply_x3(rows, M):
    """ab_bn_fin_apply_x3, RES 0 / 1 / 2, rows not a multiple of the four row lanes, M below and off the 32-pixel pass: bnp bit-equal to
    float64 AND to ab_bn_finalize on the same rows, the running statistics ONE update from their initial values, planes and out exact."""
    _finapp_case(rows, M, 64)


@pytest.mark.parametrize("M,C", FINAPP_BIG, ids=lambda v: str(v))
def test_bn_fin_apply_x3_many_strips_and_32_slices(M, C):
    """C = 64 with 1250 strips of 32 pixels on 1024 workgroups (the pixel loop wraps; only strip 0 may update the running statistics)
    and C = 2048 (32 channel slices, 32 strips each)."""
    assert bnfin_grid(M, C) == (1024 if C == 64 else 32 * 32) and (C != 64 or cdiv(M, 32) > 1024)
    _finapp_case(5, M, C)


def test_bn_fin_apply_x3_refusals():
    """65 rows and C = 96 are refused with AB_ESHAPE (the caller then runs ab_bn_finalize + ab_bn_apply_x3); nothing is written."""
    from artiboost_amd import _lib as L
    for rows, C in ((65, 64), (4, 96), (0, 64)):
        assert L.lib().ab_bn_fin_apply_x3_ok(rows, C) == 0 and not bnfin_ok(rows, C)
        z = torch.zeros((max(rows, 1), C, 2), device="cuda")
        y, one = torch.zeros((32, C), device="cuda"), torch.ones(C, device="cuda")
        bnp, pl = nan(4, C), nan(2, 32, C, dtype=torch.bfloat16)
        rc = abi("ab_bn_fin_apply_x3", z, rows, 32, one, one, 0.0, 0.5, None, None, bnp, y, None, None, None, None, 32, C, 1, None, pl[0], pl[1])
        assert rc == ESHAPE, (rows, C, rc)
        torch.cuda.synchronize()
        assert bool(torch.isnan(bnp).all()) and bool(torch.isnan(pl.float()).all())
    assert L.lib().ab_bn_fin_apply_x3_ok(64, 64) == 1 and L.lib().ab_bn_fin_apply_x3_ok(1, 2048) == 1


def _bwd_x3_launch(d, M, C, relu, out, is_hi, given_part, want_dz):
    rows = given_part.shape[0] if given_part is not None else nparts(M)
    part = given_part if given_part is not None else nan(rows, C, 2)
    bwdp, dg, db, pl = nan(2, C), nan(C), nan(C), nan(2, M, C, dtype=torch.bfloat16)
    dz = nan(M, C) if want_dz else None
    call("ab_bn_bwd_x3", d.dout, out, is_hi, d.y, d.bnp, M, C, relu, part, given_part.shape[0] if given_part is not None else 0, bwdp, dg, db,
         pl[0], pl[1], dz)
    return part, bwdp, dg, db, pl, dz


@pytest.mark.parametrize("M,C,given,route", BWDX3, ids=lambda v: str(v))
def test_bn_bwd_x3_routes_and_mask_sources(M, C, given, route):
    """ab_bn_bwd_x3 on the in-kernel finalize (rows <= 64 and C % 64 == 0) and on finalize + apply (65 rows; C = 96; 70 given rows), with
    no mask, the fp32 activation, its hi plane, and the mask recomputed from y; dz_out on and off; given rows hand-reduced; C = 2048
    reduces in two slices.  dgamma, dbeta, bwdp, dz exact; dy planes exact where M is a power of two, the sum of the planes within the
    bound otherwise; the hi-plane and fp32 masks give the same bits."""
    from artiboost_amd import kernels as K
    rows = given or nparts(M)
    assert ("fin" == route) == bnfin_ok(rows, C)
    o = exact_problem(M, C, 8)
    assert_sum_conditions(o.y)
    d = _x3_dev(o)
    pow2 = (M & (M - 1)) == 0
    vc, rl = lanes(F32, min(C, 1024))
    keep = {}
    for mk in MASKS:
        relu = {"none": 0, "out": 1, "hi": 1, "recompute": 2}[mk]
        act = ref_apply(o.y, o.bnp, True, o.res if relu == 1 else None)
        mask = None if relu == 0 else (act > 0).double()
        dz, db, dg, dy = ref_bwd(o.dout, o.y, o.bnp, mask)
        actd = dev(act) if relu == 1 else None
        out = None if relu != 1 else (K.split(actd)[0].contiguous() if mk == "hi" else actd)
        gp = None
        if given:
            # hand-reduced rows: the float64 sums spread over `given` rows of integers
            gp64 = hand_part(given, C, 0, None, None, 2, kind="bwd")
            gp64[-1] = torch.stack([db, dg], -1) - gp64[:-1].sum(0)
            gp = dev(gp64)
        for want_dz in (True, False):
            part, bwdp, dgo, dbo, pl, dzo = twice(lambda: _bwd_x3_launch(d, M, C, relu, out, 1 if mk == "hi" else 0, gp, want_dz))
            w = f"bn_bwd_x3 {route} {(M, C)} given={given} mask={mk} dz={want_dz}"
            assert_bits(w + " dbeta", dbo, db)
            assert_bits(w + " dgamma", dgo, dg)
            assert_bits(w + " bwdp", bwdp, torch.stack([db, dg]))
            if not given:
                assert bool(torch.isfinite(part).all()), w + ": a partial row was not written"
                assert_bits(w + " partial rows", part.double().sum(0), torch.stack([db, dg], -1))
            if want_dz:
                assert_bits(w + " dz", dzo, dz)
            if pow2:
                assert_planes(w + " dy", pl, dy)
            else:
                _, _, e_dy = bwd_bound(o.dout, o.y, o.bnp, mask, rl, red_rows(M), exact_sums=True)
                assert_bound(w + " dy (hi + lo)", pl.float().double().sum(0), dy, e_dy + 2.0 ** -16 * dy.abs(), 4)
            keep[(mk, want_dz)] = pl
    assert torch.equal(keep[("out", True)].view(torch.int16), keep[("hi", True)].view(torch.int16)), "hi-plane mask and fp32 mask disagree"


def test_bn_bwd_x3_refuses_channel_counts_off_the_vector():
    o = exact_problem(2, 12, 0)
    d = _x3_dev(o)
    pl = nan(2, 2, 12, dtype=torch.bfloat16)
    rc = abi("ab_bn_bwd_x3", d.dout, None, 0, d.y, d.bnp, 2, 12, 0, nan(1, 12, 2), 0, nan(2, 12), nan(12), nan(12), pl[0], pl[1], None)
    assert rc == ESHAPE


@pytest.mark.parametrize("M,C", ((1000, 128), (1040, 96), (520, 1024)))
def test_x3_producers_random_class(M, C):
    """bn_fin_apply_x3 (or finalize + bn_apply_x3) and ab_bn_bwd_x3 on randn operands: planes summed against float64 within the derived
    bound plus the 2^-16 relative residue a (hi, lo) pair leaves."""
    from artiboost_amd import kernels as K
    o = _random_problem(M, C, 2, 3)
    y, eps = rdev(o.y), 1e-5
    part = K.col_stats(y)
    if bnfin_ok(part.shape[0], C):
        pl, bnp = K.bn_fin_apply_x3(y, part, M, rdev(o.gamma), rdev(o.beta), res=rdev(o.res), relu=True, eps=eps)
    else:
        bnp = K.bn_finalize(part, M, rdev(o.gamma), rdev(o.beta), eps=eps)
        pl = K.bn_apply_x3(y, bnp, res=rdev(o.res), relu=True)
    eS, eQ = stats_bound(o.y, lanes(F32, min(C, 1024))[1])
    ref, _ = ref_bnp(o.y, o.gamma, o.beta, eps)
    e_bnp = bnp_bound(o.y, o.gamma, o.beta, eps, eS, eQ)
    w = f"random x3 {(M, C)}"
    for k, name in enumerate(("scale", "shift", "mean", "invstd")):
        assert_bound(f"{w} {name}", bnp[k], ref[k], e_bnp[k], 4)
    out = ref_apply(o.y, ref, True, o.res)
    assert_bound(w + " out (hi + lo)", pl.float().double().sum(0), out, apply_bound(o.y, ref, e_bnp, o.res) + 2.0 ** -16 * out.abs(), 4)
    b64 = _cpu64(bnp)
    pre = o.y * b64[0] + b64[1]
    mask = (pre > 0).double()
    dz, db, dg, dy = ref_bwd(o.dout, o.y, b64, mask)
    dgo, dbo = nan(C), nan(C)
    dpl = K.bn_bwd_x3(rdev(o.dout), None, y, bnp, dgo, dbo, relu="recompute")
    e_db, e_dg, e_dy = bwd_bound(o.dout, o.y, b64, mask, lanes(F32, min(C, 1024))[1], red_rows(M), pre=pre)
    assert_bound(w + " dbeta", dbo, db, e_db, 4)
    assert_bound(w + " dgamma", dgo, dg, e_dg, 4)
    assert_bound(w + " dy (hi + lo)", dpl.float().double().sum(0), dy, e_dy + 2.0 ** -16 * dy.abs(), 4)


# ---------------------------------------------------------------- 5. the stem pool
@functools.lru_cache(maxsize=None)
def pool_problem(shape):
    """Exact-class operands of maxpool3x3/2(relu(bn(y))) and its backward for one (N, H, W, C), with the float64 results."""
    N, H, W, C = shape
    M = N * H * W
    o = exact_problem(M, C, 11)
    assert_sum_conditions(o.y)
    o.shape = shape
    o.y4 = o.y.reshape(N, H, W, C)
    o.pre = o.y4 * o.bnp[0] + o.bnp[1]
    o.act = o.pre.clamp_min(0.0)
    o.pooled, o.code, o.flat = ref_pool(o.act)
    o.ywin = pool_gather(o.y4, o.flat)
    o.raw_pooled, o.raw_code, o.raw_flat = ref_pool(o.y4)
    g = _gen(*shape, 12)
    o.dpool = _ints(g, -3, 3, (N, H // 2, W // 2, C))
    o.da = pool_scatter(o.dpool, o.flat, H, W)
    o.mask = (o.pre > 0).double()
    o.dz, o.db, o.dg, o.dy = ref_bwd(o.da, o.y4, o.bnp, o.mask)
    o.raw_dx = pool_scatter(o.dpool, o.raw_flat, H, W)
    return o


def _pool_dy_check(w, o, got, planes, dt=F32):
    """dy of the pool backward: exact where N * H * W is a power of two, within the bound otherwise."""
    N, H, W, C = o.shape
    M = N * H * W
    if (M & (M - 1)) == 0:
        if planes:
            assert_planes(w + " dy", got, o.dy)
        else:
            assert_bits(w + " dy", got, rounded(o.dy, dt))
        return
    flat = lambda t: t.reshape(M, C)          # noqa: E731
    _, _, e_dy = bwd_bound(flat(o.da), flat(o.y4), o.bnp, flat(o.mask), 1, M, exact_sums=True)
    e_dy = e_dy.reshape(o.dy.shape)
    if planes:
        assert_bound(w + " dy (hi + lo)", got.float().double().sum(0), o.dy, e_dy + 2.0 ** -16 * o.dy.abs(), 5)
    else:
        assert_bound(w + " dy", got, o.dy, e_dy + (2.0 ** -8 * o.dy.abs() if dt == BF16 else 0.0), 5)


@pytest.mark.parametrize("shape", POOL, ids=lambda v: "x".join(map(str, v)))
def test_stem_pool_generic_dtypes(shape):
    """ab_maxpool3x3s2_fwd / _bwd on the raw tensor, ab_bn_relu_maxpool3x3s2_fwd and ab_bn_relu_maxpool_bwd, fp32 and (C % 8 == 0) bf16:
    pooled values, winner codes under ties of non-zero values, the scattered gradient, dgamma / dbeta and the row count exact."""
    N, H, W, C = shape
    o = pool_problem(shape)
    Ho, Wo, M = H // 2, W // 2, N * H * W
    for dt in (F32, BF16):
        if C % VEC[dt]:
            continue
        y, bnp, dpool = dev(o.y4, dt), dev(o.bnp), dev(o.dpool, dt)
        w = f"pool<{dt}> {shape}"

        def fwd(fn, *pre):
            def launch():
                out, idx = nan(N, Ho, Wo, C, dtype=TD[dt]), nan(N, Ho, Wo, C, dtype=torch.uint8)
                call(fn, y, *pre, DTC(dt), N, H, W, C, out, idx)
                return out, idx
            return twice(launch)

        out, idx = fwd("ab_maxpool3x3s2_fwd")
        assert_bits(w + " raw pooled", out, o.raw_pooled)
        assert_bits(w + " raw winners", idx, o.raw_code.double())
        dx = nan(N, H, W, C, dtype=TD[dt])
        call("ab_maxpool3x3s2_bwd", idx, dpool, DTC(dt), N, H, W, C, dx)
        assert_bits(w + " raw dx", dx, o.raw_dx)
        out, idx = fwd("ab_bn_relu_maxpool3x3s2_fwd", bnp)
        assert_bits(w + " pooled", out, o.pooled)
        assert_bits(w + " winners", idx, o.code.double())

        def bwd():
            part, bwdp, dg, db, dy = nan(nparts(M), C, 2), nan(2, C), nan(C), nan(C), nan(N, H, W, C, dtype=TD[dt])
            call("ab_bn_relu_maxpool_bwd", dpool, idx, y, bnp, DTC(dt), N, H, W, C, part, bwdp, dg, db, dy)
            return part, bwdp, dg, db, dy

        part, bwdp, dg, db, dy = twice(bwd)
        assert bool(torch.isfinite(part).all())
        assert_bits(w + " dbeta", db, o.db)
        assert_bits(w + " dgamma", dg, o.dg)
        assert_bits(w + " partial rows", part.double().sum(0), torch.stack([o.db, o.dg], -1))
        _pool_dy_check(w, o, dy, False, dt)


@pytest.mark.parametrize("shape", POOL, ids=lambda v: "x".join(map(str, v)))
def test_stem_pool_split_planes(shape):
    """ab_bn_relu_maxpool3x3s2_fwd_x3 (C % 8 == 4: the generic kernel with planes), _fwd_x3w (ywin; out = NULL), ab_bn_relu_maxpool_bwd_x3
    and _bwd_x3w; where ab_bn_relu_maxpool_bwd_x3_nparts is 0 the wrapper returns None and the route hybridnet.py then takes (max-pool
    backward + bn_bwd_x3 with the recomputed mask) is run and checked instead."""
    from artiboost_amd import _lib as L
    from artiboost_amd import kernels as K
    N, H, W, C = shape
    o = pool_problem(shape)
    Ho, Wo, M, Mp = H // 2, W // 2, N * H * W, N * (H // 2) * (W // 2)
    y, bnp, dpool = dev(o.y4), dev(o.bnp), dev(o.dpool)
    w = f"pool x3 {shape}"

    def fwd():
        out, pl, idx = nan(N, Ho, Wo, C), nan(2, N, Ho, Wo, C, dtype=torch.bfloat16), nan(N, Ho, Wo, C, dtype=torch.uint8)
        call("ab_bn_relu_maxpool3x3s2_fwd_x3", y, bnp, N, H, W, C, out, pl[0], pl[1], idx)
        return out, pl, idx

    out, pl, idx = twice(fwd)
    assert_bits(w + " pooled", out, o.pooled)
    assert_bits(w + " winners", idx, o.code.double())
    assert_planes(w + " planes", pl, o.pooled)
    rows = pool_rows(N, H, W, C)
    assert L.lib().ab_bn_relu_maxpool_bwd_x3_nparts(N, H, W, C) == rows
    if C % 8:
        ywin = nan(N, Ho, Wo, C)
        assert abi("ab_bn_relu_maxpool3x3s2_fwd_x3w", y, bnp, N, H, W, C, out, pl[0], pl[1], idx, ywin) == ESHAPE
        dgo, dbo = nan(C), nan(C)
        assert K.bn_relu_maxpool_bwd_x3(dpool, idx, y, bnp, dgo, dbo) is None
        return
    for want_out in (True, False):
        def fwdw():
            outw = nan(N, Ho, Wo, C) if want_out else None
            plw, idxw, ywin = nan(2, N, Ho, Wo, C, dtype=torch.bfloat16), nan(N, Ho, Wo, C, dtype=torch.uint8), nan(N, Ho, Wo, C)
            call("ab_bn_relu_maxpool3x3s2_fwd_x3w", y, bnp, N, H, W, C, outw, plw[0], plw[1], idxw, ywin)
            return outw, plw, idxw, ywin

        outw, plw, idxw, ywin = twice(fwdw)
        ww = w + f" x3w out={'f32' if want_out else 'NULL'}"
        if want_out:
            assert_bits(ww + " pooled", outw, o.pooled)
        assert_bits(ww + " winners", idxw, o.code.double())
        assert_planes(ww + " planes", plw, o.pooled)
        assert_bits(ww + " ywin", ywin, o.ywin)

    def bwdw():
        part, bwdp, dg, db, dpl = nan(nparts(Mp), C, 2), nan(2, C), nan(C), nan(C), nan(2, N, H, W, C, dtype=torch.bfloat16)
        call("ab_bn_relu_maxpool_bwd_x3w", dpool, idx, ywin, y, bnp, N, H, W, C, part, bwdp, dg, db, dpl[0], dpl[1])
        return part, bwdp, dg, db, dpl

    def bwd3():
        part, bwdp, dg, db, dpl = nan(rows, C, 2), nan(2, C), nan(C), nan(C), nan(2, N, H, W, C, dtype=torch.bfloat16)
        dz = nan(N, H, W, C)
        call("ab_bn_relu_maxpool_bwd_x3", dpool, idx, y, bnp, N, H, W, C, part, bwdp, dg, db, dz, dpl[0], dpl[1])
        return part, bwdp, dg, db, dpl

    def fallback():
        # hybridnet.py, _backward_trunk: dy0 is None -> K.maxpool_bwd + bn_bwd_x3(relu="recompute")
        dg, db = nan(C), nan(C)
        assert K.bn_relu_maxpool_bwd_x3(dpool, idx, y, bnp, dg, db) is None
        da = K.maxpool_bwd(idx, dpool, (H, W))
        assert_bits(w + " fallback max-pool backward", da, o.da)
        dpl = K.bn_bwd_x3(da, None, y, bnp, dg, db, relu="recompute")
        return None, None, dg, db, dpl

    for name, launch in (("x3w", bwdw), ("x3", bwd3 if rows else fallback)):
        part, bwdp, dg, db, dpl = twice(launch)
        ww = f"{w} bwd {name}" + ("" if rows or name == "x3w" else " (nparts = 0: fallback)")
        assert_bits(ww + " dbeta", db, o.db)
        assert_bits(ww + " dgamma", dg, o.dg)
        if part is not None:
            assert bool(torch.isfinite(part).all()), ww + ": a partial row was not written"
            assert_bits(ww + " partial rows", part.double().sum(0), torch.stack([o.db, o.dg], -1))
            assert_bits(ww + " bwdp", bwdp, torch.stack([o.db, o.dg]))
        _pool_dy_check(ww, o, dpl, True)
    if not rows:
        assert abi("ab_bn_relu_maxpool_bwd_x3", dpool, idx, y, bnp, N, H, W, C, nan(1, C, 2), nan(2, C), nan(C), nan(C), nan(N, H, W, C),
                   nan(N, H, W, C, dtype=torch.bfloat16), nan(N, H, W, C, dtype=torch.bfloat16)) == ESHAPE


def test_stem_pool_refusals():
    """Odd H, odd W, and C % 8 for the x3w pair: AB_ESHAPE from every pool entry point."""
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device="cuda")          # noqa: E731
    for N, H, W, C in ((1, 3, 4, 8), (1, 4, 3, 8)):
        y, bnp, o, idx = z(N, H, W, C), z(4, C), z(N, H // 2, W // 2, C), z(N, H // 2, W // 2, C, dtype=torch.uint8)
        pl, dpl = z(2, N, H // 2, W // 2, C, dtype=torch.bfloat16), z(2, N, H, W, C, dtype=torch.bfloat16)
        part, bwdp, v = z(4, C, 2), z(2, C), z(C)
        assert abi("ab_maxpool3x3s2_fwd", y, 0, N, H, W, C, o, idx) == ESHAPE
        assert abi("ab_maxpool3x3s2_bwd", idx, o, 0, N, H, W, C, y) == ESHAPE
        assert abi("ab_bn_relu_maxpool3x3s2_fwd", y, bnp, 0, N, H, W, C, o, idx) == ESHAPE
        assert abi("ab_bn_relu_maxpool3x3s2_fwd_x3", y, bnp, N, H, W, C, o, pl[0], pl[1], idx) == ESHAPE
        assert abi("ab_bn_relu_maxpool3x3s2_fwd_x3w", y, bnp, N, H, W, C, o, pl[0], pl[1], idx, o) == ESHAPE
        assert abi("ab_bn_relu_maxpool_bwd", o, idx, y, bnp, 0, N, H, W, C, part, bwdp, v, v, y) == ESHAPE
        assert abi("ab_bn_relu_maxpool_bwd_x3", o, idx, y, bnp, N, H, W, C, part, bwdp, v, v, y, dpl[0], dpl[1]) == ESHAPE
        assert abi("ab_bn_relu_maxpool_bwd_x3w", o, idx, o, y, bnp, N, H, W, C, part, bwdp, v, v, dpl[0], dpl[1]) == ESHAPE
    N, H, W, C = 1, 4, 4, 12
    y, bnp, o, idx = z(N, H, W, C), z(4, C), z(N, 2, 2, C), z(N, 2, 2, C, dtype=torch.uint8)
    dpl = z(2, N, H, W, C, dtype=torch.bfloat16)
    assert abi("ab_bn_relu_maxpool_bwd_x3w", o, idx, o, y, bnp, N, H, W, C, z(1, C, 2), z(2, C), z(C), z(C), dpl[0], dpl[1]) == ESHAPE
    assert abi("ab_maxpool3x3s2_fwd", y, 0, N, H, W, 6, o, idx) == ESHAPE


# ---------------------------------------------------------------- 6. average pool and the packing kernels
@pytest.mark.parametrize("shape", AVG, ids=lambda v: "x".join(map(str, v)))
def test_avgpool_fwd(shape):
    """ab_avgpool_fwd: exact on integers where HW is a power of two; otherwise within (ceil(HW / 8) + 8 + 1) u sum |x| / HW + u |out| (eight
    pixel lanes, an eight-term combine, one division)."""
    N, HW, C = shape
    x = _ints(_gen(*shape, 21), -3, 3, (N, HW, C))
    ref = x.sum(1) / HW
    for dt in (F32, BF16):
        if C % VEC[dt]:
            assert abi("ab_avgpool_fwd", torch.zeros((N, HW, C), dtype=TD[dt], device="cuda"), DTC(dt), N, HW, C, nan(N, C)) == ESHAPE
            continue
        xd = dev(x, dt)

        def run():
            out = nan(N, C)
            call("ab_avgpool_fwd", xd, DTC(dt), N, HW, C, out)
            return (out,)

        (out,) = twice(run)
        if (HW & (HW - 1)) == 0:
            assert_bits(f"avgpool_fwd<{dt}> {shape}", out, ref)
        else:
            assert_bound(f"avgpool_fwd<{dt}> {shape}", out, ref, (cdiv(HW, 8) + 9) * U * x.abs().sum(1) / HW + U * ref.abs(), 6)
    assert abi("ab_avgpool_fwd", torch.zeros((1, 4, 6), device="cuda"), 0, 1, 4, 6, nan(1, 6)) == ESHAPE


def test_avgpool_fwd_random_class():
    N, HW, C = 3, 49, 132
    x = torch.randn((N, HW, C), generator=_gen(5, 5), dtype=torch.float64).float().double() + 2.0
    out = nan(N, C)
    call("ab_avgpool_fwd", rdev(x), 0, N, HW, C, out)
    ref = x.sum(1) / HW
    assert_bound(f"avgpool_fwd<f32> random {(N, HW, C)}", out, ref, (cdiv(HW, 8) + 9) * U * x.abs().sum(1) / HW + U * ref.abs(), 6)


@pytest.mark.parametrize("dt", (F32, BF16))
def test_relu_bwd_and_add(dt):
    """ab_relu_bwd and ab_add, bit-equal to torch on the CPU, n below / off / above one workgroup; n % V is refused."""
    from artiboost_amd import kernels as K
    V = VEC[dt]
    for n in (V, 255 * V, 256 * V + V, 40000 * V):
        g = _gen(n, 31)
        a, b = _ints(g, -3, 3, (n,)), _ints(g, -3, 3, (n,))
        act = _ints(g, -1, 1, (n,)).clamp_min(0.0) * 0.5          # exact zeros and positives; -0.0 is not > 0 either
        act[0] = -0.0
        ad, bd, actd = dev(a, dt), dev(b, dt), act.to(TD[dt]).cuda()
        (dz,) = twice(lambda: (K.relu_bwd(ad, actd),))
        (sm,) = twice(lambda: (K.add(ad, bd),))
        assert_bits(f"relu_bwd<{dt}> n={n}", dz, torch.where(act > 0, a, torch.zeros_like(a)))
        assert_bits(f"add<{dt}> n={n}", sm, a + b)
    z = torch.zeros(V + 1, dtype=TD[dt], device="cuda")
    assert abi("ab_relu_bwd", z, z, DTC(dt), V + 1, z) == ESHAPE and abi("ab_add", z, z, DTC(dt), V + 1, z) == ESHAPE


def cast_vectors(n):
    """fp32 inputs for the cast: round-to-nearest-even ties both ways, values next to a tie, both infinities, +-0, the largest finite
    value (rounds to infinity), then randn."""
    bits = [0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000,
            0x7F7FFFFF, 0x7F7F7FFF, 0x40490FDB, 0xC0490FDB]
    head = torch.tensor([b - (1 << 32) if b >= (1 << 31) else b for b in bits], dtype=torch.int32).view(torch.float32)
    rest = torch.randn(max(n - len(bits), 0), generator=_gen(n, 41))
    return torch.cat([head, rest])[:max(n, len(bits))]


@pytest.mark.parametrize("n", (14, 255, 257, 2097155))
def test_cast_f32_bf16(n):
    """ab_cast_f32_bf16 == tensor.to(bfloat16) bit for bit, ties, infinities, n not a multiple of 256 and n past the 8192-workgroup grid; the bytes behind n stay."""
    from artiboost_amd import kernels as K
    src = cast_vectors(n)
    n = src.numel()
    dst = torch.full((n + 64,), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    K.cast_bf16(src.cuda(), dst[:n])
    exp = src.to(torch.bfloat16)
    assert torch.equal(dst[:n].cpu().view(torch.int16), exp.view(torch.int16))
    assert bool((dst[n:].view(torch.int16) == 0x5A5A).all())
    TALLY["exact"] += 1


@pytest.mark.parametrize("O,Kk,I", ((1, 1, 1), (5, 9, 7), (64, 9, 24), (40, 1, 300)))
def test_transpose_oki_single_tensor(O, Kk, I):
    """ab_transpose_oki: [O][K][I] -> [I][K][O], fp32 (a permute, any values) and bf16 (rounded like .to(bfloat16))."""
    from artiboost_amd import kernels as K
    src = torch.randn((O, Kk, I), generator=_gen(O, Kk, I))
    for dtype in (torch.float32, torch.bfloat16):
        (dst,) = twice(lambda: (K.transpose_oki(src.cuda(), nan(I, Kk, O, dtype=dtype)),))
        exp = src.permute(2, 1, 0).contiguous().to(dtype)
        assert torch.equal(dst.cpu().view(torch.int16 if dtype == torch.bfloat16 else torch.int32), exp.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
        TALLY["exact"] += 1


@pytest.mark.parametrize("N,H,W", ((1, 1, 1), (2, 5, 7), (3, 32, 48)))
def test_image_pad_nhwc4(N, H, W):
    """ab_image_pad_nhwc4: NCHW [N, 3, H, W] -> NHWC4 [N, H + 6, W + 8, 4], 3 pixels of zero border in front, channel 3 zero."""
    from artiboost_amd import kernels as K
    img = torch.randn((N, 3, H, W), generator=_gen(N, H, W, 51))
    for dtype in (torch.float32, torch.bfloat16):
        (out,) = twice(lambda: (K.image_pad_nhwc4(img.cuda(), dtype),))
        exp = torch.zeros((N, H + 6, W + 8, 4), dtype=torch.float32)
        exp[:, 3:3 + H, 3:3 + W, :3] = img.permute(0, 2, 3, 1)
        exp = exp.to(dtype)
        assert torch.equal(out.cpu().view(torch.int16 if dtype == torch.bfloat16 else torch.int32), exp.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
        TALLY["exact"] += 1


# ---------------------------------------------------------------- 7. guarded tails
TAIL, PRE = 4096, 1040


def guarded(shape, dtype=torch.float32):
    """A view of `shape` inside a byte buffer of 0xA5, 1040 bytes in, with 4 KiB behind it."""
    n = torch.empty((), dtype=dtype).element_size()
    for v in shape:
        n *= v
    buf = torch.full((PRE + n + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[PRE:PRE + n].view(dtype).view(shape)


class Guards:
    def __init__(self):
        self.bufs = []

    def new(self, name, shape, dtype=torch.float32):
        buf, view = guarded(shape, dtype)
        self.bufs.append((name, buf, view.numel() * view.element_size()))
        return view

    def check(self, what):
        torch.cuda.synchronize()
        for name, buf, n in self.bufs:
            assert bool((buf[:PRE] == 0xA5).all()), f"{what}: wrote in front of its {name}"
            assert bool((buf[PRE + n:] == 0xA5).all()), f"{what}: wrote behind its {name}"


def test_guarded_tails_batchnorm_family():
    """M = 33, C = 96 (one-row last block, 16 idle lanes, per-iteration parameters): every output of the statistics, finalize, apply and
    backward entry points, generic and split-plane, written into a slice of a larger buffer; the bytes around each slice stay 0xA5."""
    M, C = 33, 96
    o = exact_problem(M, C, 13, balanced=False)
    bh = torch.bfloat16
    for dt in (F32, BF16):
        G = Guards()
        y, res, dout, bnp = dev(o.y, dt), dev(o.res, dt), dev(o.dout, dt), dev(o.bnp)
        rows = nparts(M)
        part, tot = G.new("partial rows", (rows, C, 2)), G.new("column sums", (C,))
        call("ab_col_sum", y, DTC(dt), M, C, part, tot)
        assert_bits(f"guarded col_sum<{dt}>", tot, o.y.sum(0))
        fb = G.new("bnp", (4, C))
        rm, rv = G.new("running_mean", (C,)), G.new("running_var", (C,))
        rm.zero_(), rv.fill_(1.0)
        call("ab_bn_finalize", part, rows, C, M, dev(o.gamma), dev(o.beta), 1e-5, 0.5, rm, rv, fb)
        out = G.new("out", (M, C), TD[dt])
        call("ab_bn_apply", y, res, bnp, DTC(dt), M, C, 1, out)
        ref = ref_apply(o.y, o.bnp, True, o.res)
        assert_bits(f"guarded bn_apply<{dt}>", out, ref)
        bpart, bwdp, dg, db = G.new("backward rows", (rows, C, 2)), G.new("bwdp", (2, C)), G.new("dgamma", (C,)), G.new("dbeta", (C,))
        dy, dzo = G.new("dy", (M, C), TD[dt]), G.new("dz", (M, C), TD[dt])
        call("ab_bn_bwd", dout, out, y, bnp, DTC(dt), M, C, 1, bpart, bwdp, dg, db, dy, dzo)
        dz, rdb, rdg, _ = ref_bwd(o.dout, o.y, o.bnp, (ref > 0).double())
        assert_bits(f"guarded bn_bwd<{dt}> dz", dzo, dz)
        assert_bits(f"guarded bn_bwd<{dt}> dgamma", dg, rdg)
        if dt == F32:
            o3, hi, lo = G.new("x3 out", (M, C)), G.new("hi plane", (M, C), bh), G.new("lo plane", (M, C), bh)
            call("ab_bn_apply_x3", y, res, bnp, M, C, 1, o3, hi, lo)
            assert_bits("guarded bn_apply_x3", o3, ref)
            assert_bits("guarded bn_apply_x3 hi + lo", hi.double() + lo.double(), ref)
            dh, dl, dz3 = G.new("dy hi", (M, C), bh), G.new("dy lo", (M, C), bh), G.new("x3 dz", (M, C))
            call("ab_bn_bwd_x3", dout, hi, 1, y, bnp, M, C, 1, bpart, 0, bwdp, dg, db, dh, dl, dz3)
            assert_bits("guarded bn_bwd_x3 dz", dz3, dz)
            assert_bits("guarded bn_bwd_x3 dbeta", db, rdb)
        G.check(f"BatchNorm family <{dt}> {(M, C)}")
    # the in-kernel finalize: M = 33, C = 64, 3 rows
    C, rows, count = 64, 3, 12
    p = _fin_problem(rows, C, count, 1)
    y = p.mu + p.sigma * exact_problem(M, C, 14, balanced=False).s
    G = Guards()
    fb, rm, rv = G.new("bnp", (4, C)), G.new("running_mean", (C,)), G.new("running_var", (C,))
    rm.copy_(dev(p.rm0)), rv.copy_(dev(p.rv0))
    o3, hi, lo = G.new("out", (M, C)), G.new("hi plane", (M, C), bh), G.new("lo plane", (M, C), bh)
    call("ab_bn_fin_apply_x3", dev(p.part), rows, count, dev(p.gamma), dev(p.beta), 0.0, 0.5, rm, rv, fb, dev(y), None, None, None, None, M, C, 1, o3, hi, lo)
    assert_bits("guarded bn_fin_apply_x3 bnp", fb, p.bnp)
    assert_bits("guarded bn_fin_apply_x3 out", o3, ref_apply(y, p.bnp, True))
    assert_running_once("guarded bn_fin_apply_x3", rm, rv, p.rm0, p.rv0, p.mu, p.sigma ** 2, count, 0.5)
    G.check("bn_fin_apply_x3 (33, 64)")


def test_guarded_tails_pool_family():
    """(2, 10, 6, 64), Ho = 5 (a partial last group of PFX_ROWS rows): the pool entry points, generic and split-plane, forward and backward,
    and the average pool, on sliced outputs."""
    shape = (2, 10, 6, 64)
    N, H, W, C = shape
    Ho, Wo, M, Mp = H // 2, W // 2, N * H * W, N * (H // 2) * (W // 2)
    o = pool_problem(shape)
    bh = torch.bfloat16
    y, bnp, dpool = dev(o.y4), dev(o.bnp), dev(o.dpool)
    G = Guards()
    out, idx = G.new("pooled", (N, Ho, Wo, C)), G.new("winners", (N, Ho, Wo, C), torch.uint8)
    call("ab_bn_relu_maxpool3x3s2_fwd", y, bnp, 0, N, H, W, C, out, idx)
    assert_bits("guarded pool fwd", out, o.pooled)
    hi, lo, yw = G.new("hi plane", (N, Ho, Wo, C), bh), G.new("lo plane", (N, Ho, Wo, C), bh), G.new("ywin", (N, Ho, Wo, C))
    out3, idx3 = G.new("x3 pooled", (N, Ho, Wo, C)), G.new("x3 winners", (N, Ho, Wo, C), torch.uint8)
    call("ab_bn_relu_maxpool3x3s2_fwd_x3w", y, bnp, N, H, W, C, out3, hi, lo, idx3, yw)
    assert_bits("guarded pool fwd x3w", out3, o.pooled)
    assert_bits("guarded pool fwd x3w winners", idx3, o.code.double())
    assert_bits("guarded pool fwd x3w ywin", yw, o.ywin)
    dx = G.new("dx", (N, H, W, C))
    call("ab_maxpool3x3s2_bwd", idx, dpool, 0, N, H, W, C, dx)
    assert_bits("guarded pool bwd", dx, o.da)
    rows = pool_rows(N, H, W, C)
    part, bwdp, dg, db = G.new("pool rows", (rows, C, 2)), G.new("bwdp", (2, C)), G.new("dgamma", (C,)), G.new("dbeta", (C,))
    dz, dh, dl = G.new("dz scratch", (N, H, W, C)), G.new("dy hi", (N, H, W, C), bh), G.new("dy lo", (N, H, W, C), bh)
    call("ab_bn_relu_maxpool_bwd_x3", dpool, idx, y, bnp, N, H, W, C, part, bwdp, dg, db, dz, dh, dl)
    assert_bits("guarded pool bwd x3 dgamma", dg, o.dg)
    partw = G.new("pooled rows", (nparts(Mp), C, 2))
    call("ab_bn_relu_maxpool_bwd_x3w", dpool, idx, yw, y, bnp, N, H, W, C, partw, bwdp, dg, db, dh, dl)
    assert_bits("guarded pool bwd x3w dbeta", db, o.db)
    partg, dyg = G.new("generic rows", (nparts(M), C, 2)), G.new("generic dy", (N, H, W, C))
    call("ab_bn_relu_maxpool_bwd", dpool, idx, y, bnp, 0, N, H, W, C, partg, bwdp, dg, db, dyg)
    assert_bits("guarded pool bwd generic dgamma", dg, o.dg)
    avg = G.new("average", (N, C))
    call("ab_avgpool_fwd", y, 0, N, H * W, C, avg)
    G.check(f"pool family {shape}")


def test_zz_report():
    """Prints what the docstring's "Observed" block records (run the file with -s)."""
    print(f"\nexact comparisons bit-equal: {TALLY['exact']}")
    for sec, (r, what) in sorted(TALLY["ratio"].items(), key=lambda kv: str(kv[0])):
        print(f"largest err/bound, section {sec}: {r:.4f}  {what}")
    for ratio, (rel, bound) in sorted(OFFSET_REPORT.items()):
        print(f"offset ratio {ratio}: invstd relative error {rel:.3e}, first-order bound {bound:.3e}")
