"""Every soft-argmax head kernel form of softargmax.hip against torch-CPU float64, reached by shape alone at the defaults.

No test here sets an environment switch.  Every case names the code ab_softargmax3d_form must return for it -- the launchers switch on that
same function -- and asserts it before the launch.  The reference is learner_oracle.softargmax3d on the float64 upcast of exactly the values
the kernel reads (for bf16 the bf16-rounded logits); padded depth slots hold 7.0 on the device and are stripped before the reference sees the
logits; gradients are float64 autograd of sum(uvd * g_uvd) [+ sum(conf * g_conf)].  Logits are 3 * randn (test_gpu_head.py's scale, so its
tolerances apply); bf16 logits carry one planted maximum per class (max + 1) so that the confidence gradient has one taker.

Form table (ab_softargmax3d_form: entry 0 = forward stage 1, 1 = backward, 2 = split-plane backward, 3 = split-plane backward + bias):
  section 1  entry 0, f32 | bf16, softmax | sigmoid
               10   sam_stage1_scalar                 C*DP = 1, 15 (DP > D), 33 (D = 33), 45, 1023 (all 16 channel slots of a lane)
               121  sam_stage1<*, 2, *>, 32-lane merge  C*DP = 2 (the CD - 2 clamp), 256;     120  one thread per class: 102 (D = 33, DP = 34)
               141  sam_stage1<*, 4, *>                 C*DP = 264 (DP > D), 512;             140  258 (D = 43)
               161  sam_stage1<*, 6, *>                 C*DP = 616, 704 (28 in 32), 768;      160  514 (D = 257)
               181  sam_stage1<*, 8, *>                 C*DP = 1012 (D = 28, DP = 46), 1024;  180  770 (D = 35)
             pixels 1 x 1 (three waves of the tile idle), 1 x 3 (one wave idle), 63, 64, 65, 1 x 65, 65 x 1, 7 x 5, 72 x 72 (81 tiles:
             sam_stage2's lane-strided loop takes its second trip), B in {1, 3}
  section 2  ab_softargmax3d_stage2 alone on the forward's part buffer: 1, 2 and 81 tiles, bit-equal to the forward's outputs
  section 3  entry 1, f32 | bf16, softmax (with and without g_conf) | sigmoid
               20    sam_bwd_scalar                      C*DP = 1, 15, 45
               1628  sam_bwd<T, false, 16, N, 2, 8>      C*DP = 2, 50, 616, 1022, 1024;  pixels 1, 15, 16, 17, 63, 64, 65
             inplace = True bit-equal to out of place; padded depth slots of dlogits exactly 0
  section 4  entries 2 and 3, softmax (with and without g_conf) | sigmoid, every case through both entries
               11643 / 16443  sam_bwd<float, true, 16 | 64, N, 4, 3>   C*DP = 4, 704, 768
               11644 / 16444  sam_bwd<float, true, 16 | 64, N, 4, 4>   C*DP = 772, 1024
               11628 / 16428  sam_bwd<float, true, 16 | 64, N, 2, 8>   C*DP = 2, 50, 770, 1022
             pixels 1, 15, 16, 17, 63, 64, 65, 5184;  colpart rows 1, 2, 3, 32, 33, 243 through sam_bias_finalize;  hi + lo (summed in
             float64) against the reference gradient, dbias against the float64 column sums of the REFERENCE gradient, and the planes
             of the bias call bit-equal to the plain call's
  section 5  sigmoid head at small weight sums: logits = -20 + randn on 4 x 4 x 4 and 2 x 3 x 5 volumes, C*DP even and odd, forward and
             the f32, bf16 and split-plane backwards (1e-7 / S between 0.30 and 1.44 here; the host file asserts > 0.05)
  section 6  refusals: C*DP > 1024, DP < D, odd C*DP on entries 2 and 3 (AB_ESHAPE), g_conf with norm = 1 (AB_EINVAL); sentinels untouched
  section 7  guarded 4 KiB of 0xA5 either side of every output, once per kernel family (the GUARDED table names the four forms of each case)
  Every launch of sections 1 - 5 and 7 -- the forwards that only feed a backward or stage 2, the in-place backward and the guarded
  launches included -- is repeated once into fresh outputs and must be bit-equal to itself; each is preceded by the assertion of its form.

Not reachable by shape: AB_SAM_BWD_QUAD=0 (entries 2 and 3 take <2, 8> at every even C*DP; the same instantiation is in the table at
  C*DP % 4 != 0).  The fused final-layer route (ab_conv1x1_sam_fwd_x3) is pinned in test_gpu_fwd_dgrad.py and test_gpu_conv_x3.py.

Bounds (test_gpu_head.py::test_head_vs_oracle and its neighbours): uvd atol 3e-6;  conf rtol 3e-5 + atol 1e-8;  fp32 dlogits rtol 1e-4 + atol
  1e-5 max|ref|;  bf16-stored dlogits rtol 1e-2 + atol 1e-2 max|ref| (the 2^-8 store rounding is the bound);  hi + lo rtol 2e-4 + atol 2e-5
  max|ref|;  dbias 2e-6 x the largest column sum of |ref|.  The small-S cases use the same forms, except conf: max sigmoid(x) is about
  2e-8 there and the absolute 1e-8 would allow half of it, so section 5 asserts rtol 3e-5 alone (atol 0; stricter, reasoned in
  check_forward: two half-ulp roundings of log sigmoid(x) near -20 and the exponential cost about 2e-6 relative).  stat[..., 0] of the softmax head is the
  maximum logit itself and is compared exactly.

Known deviations.
  Confidence gradient on ties: the kernels give the g_conf term to EVERY voxel that ties for the class maximum ((xp == m ? 1 : 0)); the
  reference's torch.max(dim) hands its gradient to the first maximal index only.  Resolving it needs the arg-max index in `stat` (a layout
  change); every g_conf input here has one maximum per class, asserted on the reference side.
  The confidence gradient of the sigmoid head is refused (AB_EINVAL), not computed.

Observed on an MI355X.
  212 tests, 3.4 s for the file (the slowest case 0.34 s: the first launch; the 21 MB case 0.1 s).  346 comparisons against float64, 383
  bit-equal comparisons (stage 2 alone, in place, bias-call planes, guarded against unguarded, stat maxima), 539 repeated launches
  all bit-equal to the first, every refusal with its code and its sentinels intact, no guarded byte changed.
  Largest err / tol:  section 1  0.162  form 180 f32 softmax [C*DP=770; D=35; 65 pixels] uvd
                      section 3  0.183  form 1628 bf16 sigmoid [C*DP=616; 63 pixels] dlogits (the bf16 store rounding)
                      section 4  0.888  form 16443 softmax+g_conf [C*DP=4; 1 pixel; rows=3] dbias (three addends: the fp32 error of
                                        dlogits itself against a bound meant for long column sums); next 0.579, form 16444 C*DP=1024
                      section 5  0.142  small S f32 [4x4x4; C*DP=8 even] dbias;  dlogits 0.005 - 0.023 (f32, planes), 0.08 - 0.14 (bf16);
                                        conf under the relative bound alone 0.017 - 0.029 (largest relative error 8.7e-7)
  No case needed a bound other than the listed ones.
  Found and changed (test_sigmoid_small_weight_sum, all eight cases): both backward kernels used the softmax constants for the sigmoid
  head -- 1 / (s (1 + 1e-7)) as the per-class factor and uvd (1 + 1e-7) as the centre -- where the reference divides by S + 1e-7 with
  S = sum w.  Against float64 the gradient of the parent commit was off by 0.34, 0.32, 0.95 and 0.77 of max|ref| on the four small-S
  shapes (f32, and the same through the split planes); with w_max / (s w_max + 1e-7) and uvd itself it is 4.4e-7, 1.9e-7, 2.3e-7,
  1.8e-7 (planes 2.3e-6, 1.3e-6).  At 3 * randn (S >> 1e-7) the sigmoid gradient moved by 4.5e-7 of its maximum.  The softmax
  instantiations did not change: built from the parent commit and from this one, uvd, conf, stat, dlogits (f32 and bf16, with and
  without g_conf), both plane pairs and dbias are bit-equal at 22 x 28 in a pitch of 32 on 8 x 8 (B = 3) and at C*DP = 616, 45, 1024
  and 1022, and all 32 forward and softmax-backward kernels compile to the same instructions.  Nothing else differed from its reference.
  Sensitivity: against a build of softargmax.hip with five planted arithmetic errors (the D > 32 merge skipping the last depth bin,
  sam_stage1<*, 8, *> dropping asv from its rescale, sam_bwd<.., 4, 4> using ca for cb, sam_stage2 skipping tiles >= 64,
  sam_bias_finalize starting its row loop at pl + 32) 89 of the 212 tests fail and each of the five fails at least one: all 16 cases of
  forms 120 / 140 / 160 / 180, the 8 cases of form 181 with more than one pixel group (63 pixels, 81 tiles), the other 8 cases with 81
  tiles, all 45 split-plane cases and the 2 even small-S f32 cases on dbias (the 9 cases of forms 11644 / 16444 already on hi + lo).
  Failing without their own form being one of the five: 10 of the 12 section 3 cases at C*DP = 1022 and 1024, and hi + lo of form 11628
  at C*DP = 770, 1022 and at 5184 pixels -- the backward reads uvd and stat from the forward the test runs first, and that forward is
  form 180 / 181 or merges 81 tiles.  The other two, bf16 sigmoid at 1022 and at 1024, pass: the wrong v of uvd moves the sigmoid
  gradient little (the f32 cases of the same shapes fail at 553 and 280 times their bound), and the bf16 store bound is 100 (relative
  term) to 1000 (absolute term) times the f32 one.  Passing although they launch a planted error: form 181 at 1 x 1 (one pixel group: nothing to
  rescale), and the self-comparisons (stage 2 alone against the forward's stage 2, guarded against unguarded).
"""
import functools
import re
import types

import pytest
import torch

import learner_oracle as lo

pytestmark = pytest.mark.gpu

F32, BF16 = "f32", "bf16"
TD = {F32: torch.float32, BF16: torch.bfloat16}
NORMS = ("softmax", "sigmoid")
EINVAL, ESHAPE = -1, -2
PAD_VALUE = 7.0

# ---------------------------------------------------------------- case tables
# section 1: (form, C, D, DP, B, H, W, what)
S1 = (
    (10, 1, 1, 1, 1, 1, 1, "C*DP=1; 1x1: three waves idle"),
    (10, 3, 4, 5, 3, 7, 5, "C*DP=15; DP>D; 7x5"),
    (10, 1, 33, 33, 1, 9, 7, "C*DP=33; D=33; 63 pixels"),
    (10, 5, 9, 9, 3, 65, 1, "C*DP=45; 65x1"),
    (10, 5, 9, 9, 1, 72, 72, "C*DP=45; 81 tiles"),
    (10, 31, 33, 33, 1, 5, 13, "C*DP=1023; D=33; 65 pixels"),
    (121, 1, 2, 2, 3, 1, 1, "C*DP=2: CD-2 clamp; 1x1"),
    (121, 1, 2, 2, 1, 72, 72, "C*DP=2; 81 tiles"),
    (120, 3, 33, 34, 1, 1, 65, "C*DP=102; D=33; DP>D; 1x65"),
    (121, 8, 32, 32, 3, 8, 8, "C*DP=256; 64 pixels"),
    (140, 6, 43, 43, 1, 65, 1, "C*DP=258; D=43; 65x1"),
    (141, 11, 20, 24, 3, 7, 5, "C*DP=264; DP>D; 7x5"),
    (141, 16, 32, 32, 1, 9, 7, "C*DP=512; 63 pixels"),
    (160, 2, 257, 257, 1, 1, 3, "C*DP=514; D=257; 1x3: one wave idle"),
    (161, 22, 28, 28, 3, 7, 5, "C*DP=616; 7x5"),
    (161, 22, 28, 32, 3, 5, 13, "C*DP=704; DP>D; 65 pixels"),
    (161, 24, 32, 32, 1, 1, 1, "C*DP=768; 1x1"),
    (180, 22, 35, 35, 1, 13, 5, "C*DP=770; D=35; 65 pixels"),
    (181, 22, 28, 46, 3, 9, 7, "C*DP=1012; DP>D; 63 pixels"),
    (181, 32, 32, 32, 1, 1, 1, "C*DP=1024; 1x1"),
    (181, 32, 32, 32, 1, 72, 72, "C*DP=1024; 81 tiles"),
)
# section 2: (C, D, DP, B, H, W): ntile = 1, 2, 81
S2 = ((5, 9, 9, 3, 1, 1), (22, 28, 32, 1, 5, 13), (5, 9, 10, 3, 72, 72))
# section 3: (form, C, D, DP, B, H, W, what)
BW = (
    (20, 1, 1, 1, 1, 1, 1, "C*DP=1; 1 pixel"),
    (20, 3, 4, 5, 3, 7, 5, "C*DP=15; DP>D; 35 pixels"),
    (20, 5, 9, 9, 1, 65, 1, "C*DP=45; 65 pixels"),
    (1628, 1, 2, 2, 3, 1, 1, "C*DP=2: CD-V clamp; 1 pixel"),
    (1628, 1, 2, 2, 1, 3, 5, "C*DP=2; 15 pixels"),
    (1628, 5, 9, 10, 3, 4, 4, "C*DP=50; DP>D; 16 pixels"),
    (1628, 5, 9, 10, 1, 17, 1, "C*DP=50; DP>D; 17 pixels"),
    (1628, 22, 28, 28, 3, 9, 7, "C*DP=616; 63 pixels"),
    (1628, 73, 14, 14, 1, 8, 8, "C*DP=1022; 64 pixels"),
    (1628, 32, 32, 32, 1, 5, 13, "C*DP=1024; 65 pixels"),
)
# section 4: (form of entry 2, form of entry 3, C, D, DP, B, H, W, what); colpart rows = B * ceil(H*W / 64)
SP = (
    (11643, 16443, 1, 4, 4, 3, 1, 1, "C*DP=4; 1 pixel; rows=3"),
    (11643, 16443, 2, 2, 2, 32, 1, 1, "C*DP=4; 1 pixel; rows=32"),
    (11643, 16443, 1, 4, 4, 3, 72, 72, "C*DP=4; 5184 pixels; rows=243"),
    (11643, 16443, 22, 28, 32, 3, 8, 8, "C*DP=704; DP>D; 64 pixels; rows=3"),
    (11643, 16443, 22, 28, 32, 1, 5, 13, "C*DP=704; DP>D; 65 pixels; rows=2"),
    (11643, 16443, 24, 32, 32, 1, 3, 5, "C*DP=768; 15 pixels; rows=1"),
    (11644, 16444, 4, 190, 193, 1, 4, 4, "C*DP=772; DP>D; 16 pixels; rows=1"),
    (11644, 16444, 32, 32, 32, 1, 17, 1, "C*DP=1024; 17 pixels; rows=1"),
    (11644, 16444, 32, 32, 32, 1, 9, 7, "C*DP=1024; 63 pixels; rows=1"),
    (11628, 16428, 1, 2, 2, 33, 1, 1, "C*DP=2; 1 pixel; rows=33"),
    (11628, 16428, 1, 2, 2, 3, 72, 72, "C*DP=2; 5184 pixels; rows=243"),
    (11628, 16428, 5, 9, 10, 1, 8, 8, "C*DP=50; DP>D; 64 pixels; rows=1"),
    (11628, 16428, 5, 9, 10, 3, 72, 72, "C*DP=50; DP>D; 5184 pixels; rows=243"),
    (11628, 16428, 22, 35, 35, 1, 5, 13, "C*DP=770; 65 pixels; rows=2"),
    (11628, 16428, 73, 14, 14, 1, 1, 1, "C*DP=1022; 1 pixel; rows=1"),
)
VARIANTS = ("softmax", "softmax+g_conf", "sigmoid")
# section 5: (C, D, DP, B, H, W, what) -- logits -20 + randn, sigmoid head
SMALL_S = (
    (2, 4, 4, 2, 4, 4, "4x4x4; C*DP=8 even"),
    (3, 4, 5, 2, 4, 4, "4x4x4; C*DP=15 odd; DP>D"),
    (3, 2, 2, 2, 3, 5, "2x3x5; C*DP=6 even"),
    (3, 2, 3, 2, 3, 5, "2x3x5; C*DP=9 odd; DP>D"),
)
# section 6: (entry points, C, D, DP, with g_conf, norm, code)
REFUSALS = (
    ((0, 1, 2, 3), 33, 32, 32, False, 0, ESHAPE),      # C*DP = 1056
    ((0, 1, 2, 3), 4, 9, 8, False, 0, ESHAPE),         # DP < D
    ((2, 3), 5, 9, 9, False, 0, ESHAPE),               # odd C*DP on the split entries
    ((2, 3), 3, 3, 5, False, 1, ESHAPE),
    ((1,), 4, 8, 8, True, 1, EINVAL),                  # g_conf of the sigmoid head
    ((1,), 5, 9, 9, True, 1, EINVAL),
)
ALL_FORMS = {0: (10, 120, 121, 140, 141, 160, 161, 180, 181), 1: (20, 1628), 2: (11628, 11643, 11644), 3: (16428, 16443, 16444)}


def variant(v):
    """-> (norm code, with g_conf)"""
    return (1 if v == "sigmoid" else 0), v.endswith("g_conf")


def all_cases():
    """Every launch shape of the file as (section, entry, form, dtypes, (C, D, DP, B, H, W), variants, what)."""
    t = []
    for form, C, D, DP, B, H, W, what in S1:
        t.append((1, 0, form, (F32, BF16), (C, D, DP, B, H, W), ("softmax", "sigmoid"), what))
    for form, C, D, DP, B, H, W, what in BW:
        t.append((3, 1, form, (F32, BF16), (C, D, DP, B, H, W), VARIANTS, what))
    for f2, f3, C, D, DP, B, H, W, what in SP:
        t.append((4, 2, f2, (F32,), (C, D, DP, B, H, W), VARIANTS, what))
        t.append((4, 3, f3, (F32,), (C, D, DP, B, H, W), VARIANTS, what))
    for C, D, DP, B, H, W, what in SMALL_S:
        t.append((5, 0, restated_form(0, C, D, DP), (F32, BF16), (C, D, DP, B, H, W), ("sigmoid",), what))
        t.append((5, 1, restated_form(1, C, D, DP), (F32, BF16), (C, D, DP, B, H, W), ("sigmoid",), what))
        if (C * DP) % 2 == 0:
            t.append((5, 2, restated_form(2, C, D, DP), (F32,), (C, D, DP, B, H, W), ("sigmoid",), what))
            t.append((5, 3, restated_form(3, C, D, DP), (F32,), (C, D, DP, B, H, W), ("sigmoid",), what))
    return t


def restated_form(entry, C, D, DP):
    """The dispatch restated from the launch conditions (ab_softargmax3d_form is the authority; the host file compares the two everywhere)."""
    CD = C * DP
    if entry == 0:
        if CD % 2:
            return 10
        kp = -(-CD // 128)
        return 100 + 10 * (2 if kp <= 2 else 4 if kp <= 4 else 6 if kp <= 6 else 8) + (1 if D <= 32 else 0)
    if entry == 1:
        return 20 if CD % 2 else 1628
    vk = (43 if CD <= 768 else 44) if CD % 4 == 0 else 28
    return 10000 + (16 if entry == 2 else 64) * 100 + vk


# ---------------------------------------------------------------- operands and the float64 reference (CPU only: the host file uses them too)
def _gen(*key):
    return torch.Generator().manual_seed(sum((int(v) + 7) * 131 ** i for i, v in enumerate(key)) % (1 << 31))


@functools.lru_cache(maxsize=6)
def operands(dt, C, D, DP, B, H, W, small_s=False):
    """core: the logits the kernel reads, [B, C, D, H, W] in the kernel's dtype; g_uvd, g_conf: fp32 cotangents."""
    g = _gen(C, D, DP, B, H, W, 1 if small_s else 0)
    core = torch.randn(B, C, D, H, W, generator=g)
    core = (core - 20.0) if small_s else 3.0 * core
    core = core.to(TD[dt])
    if dt == BF16 and not small_s:                  # one clear maximum per class: bf16 logits tie often
        flat = core.reshape(B, C, -1)
        at = torch.randint(0, flat.shape[2], (B, C, 1), generator=g)
        flat.scatter_(2, at, (flat.float().amax(2, keepdim=True) + 1.0).to(TD[dt]))
        core = flat.reshape(B, C, D, H, W)
    return types.SimpleNamespace(core=core, g_uvd=torch.randn(B, C, 3, generator=g), g_conf=torch.randn(B, C, generator=g))


def unique_max(core):
    flat = core.double().reshape(core.shape[0], core.shape[1], -1)
    return bool(((flat == flat.amax(2, keepdim=True)).sum(2) == 1).all())


@functools.lru_cache(maxsize=6)
def reference(dt, C, D, DP, B, H, W, norm, with_conf=False, small_s=False, grad=True, precision=torch.float64):
    """learner_oracle.softargmax3d in `precision` on the upcast of the kernel's logits -> uvd, conf, and d loss / d logits [B, C, D, H, W]."""
    o = operands(dt, C, D, DP, B, H, W, small_s)
    x = o.core.to(precision).reshape(B, C * D, H, W).clone().requires_grad_(grad)
    uvd, conf = lo.softargmax3d(x, C, D, H, W, norm_type=NORMS[norm])
    r = types.SimpleNamespace(uvd=uvd.detach(), conf=conf.detach(), grad=None)
    if grad:
        loss = (uvd * o.g_uvd.to(precision)).sum()
        if with_conf:
            assert unique_max(o.core), "the confidence gradient needs one maximum per class"
            loss = loss + (conf * o.g_conf.to(precision)).sum()
        loss.backward()
        r.grad = x.grad.reshape(B, C, D, H, W)
    return r


def nhwc(core, DP):
    """[B, C, D, H, W] -> the device layout [B, H, W, C*DP] with PAD_VALUE in the padded depth slots."""
    B, C, D, H, W = core.shape
    pad = torch.full((B, C, DP, H, W), PAD_VALUE, dtype=core.dtype)
    pad[:, :, :D] = core
    return pad.reshape(B, C * DP, H, W).permute(0, 2, 3, 1).contiguous()


def from_nhwc(t, C, DP):
    """device [B, H, W, C*DP] -> CPU float64 [B, C, DP, H, W]"""
    B, H, W, _ = t.shape
    return t.detach().cpu().double().permute(0, 3, 1, 2).reshape(B, C, DP, H, W)


# ---------------------------------------------------------------- the C ABI
def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def abi(fn, *args, stream=True):
    """The C ABI through the package's own loader; returns the return code (the dispatcher binding raises on a non-zero code and names
    it in the message; the ctypes binding returns it)."""
    from artiboost_amd import _lib as L
    try:
        return getattr(L.lib(), fn)(*(args + ((L.stream(),) if stream else ())))
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


def witness(entry, dt, C, D, DP, norm):
    return abi("ab_softargmax3d_form", entry, DTC(dt), C, D, DP, norm, stream=False)


def expect_form(form, entry, dt, C, D, DP, norm):
    got = witness(entry, dt, C, D, DP, norm)
    assert got == form, f"entry {entry} {dt} C={C} D={D} DP={DP} norm={norm}: the table says form {form}, ab_softargmax3d_form says {got}"


def ntiles(H, W):
    return abi("ab_softargmax3d_ntiles", H, W, stream=False)


def _bytes(t):
    return torch.empty(t.numel(), dtype=t.dtype, device=t.device).copy_(t.reshape(-1)).view(torch.uint8)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(_bytes(a), _bytes(b))


def twice(launch):
    """Runs a launch twice into fresh NaN-filled outputs; the second result must be bit-equal to the first."""
    a = launch()
    b = launch()
    torch.cuda.synchronize()
    for x, z in zip(a, b):
        assert bits_equal(x, z), "a second call differs from the first"
    TALLY["repeat"] += 1
    return a


def fwd(x, C, D, DP, norm, out=None):
    """ab_softargmax3d_fwd_norm -> part, uvd, conf, stat"""
    B, H, W, _ = x.shape
    part, uvd, conf, stat = out or (nan(B, ntiles(H, W), C, 8), nan(B, C, 3), nan(B, C), nan(B, C, 2))
    call("ab_softargmax3d_fwd_norm", x, DTC(BF16 if x.dtype == torch.bfloat16 else F32), B, C, D, DP, H, W, norm, part, uvd, conf, stat)
    return part, uvd, conf, stat


def bwd(x, C, D, DP, norm, f, gu, gc, dl=None):
    B, H, W, _ = x.shape
    dl = nan(*x.shape, dtype=x.dtype) if dl is None else dl
    call("ab_softargmax3d_bwd_norm", x, DTC(BF16 if x.dtype == torch.bfloat16 else F32), B, C, D, DP, H, W, norm, f[1], f[2], f[3], gu, gc, dl)
    return (dl,)


def bwd_split(x, C, D, DP, norm, f, gu, gc, bias, out=None):
    """entries 2 / 3 -> (hi, lo[, colpart, dbias]); the sigmoid head through ab_softargmax3d_bwd_x3_norm"""
    B, H, W, _ = x.shape
    hi, lo = (nan(*x.shape, dtype=torch.bfloat16), nan(*x.shape, dtype=torch.bfloat16)) if out is None else out[:2]
    if not bias:
        if norm:
            call("ab_softargmax3d_bwd_x3_norm", x, B, C, D, DP, H, W, norm, f[1], f[2], f[3], gu, hi, lo, None, None)
        else:
            call("ab_softargmax3d_bwd_x3", x, B, C, D, DP, H, W, f[1], f[2], f[3], gu, gc, hi, lo)
        return hi, lo
    rows = abi("ab_softargmax3d_bwd_x3_bias_rows", B, H, W, stream=False)
    assert rows == B * -(-H * W // 64)
    colpart, dbias = (nan(rows, C * DP), nan(C * DP)) if out is None else out[2:]
    if norm:
        call("ab_softargmax3d_bwd_x3_norm", x, B, C, D, DP, H, W, norm, f[1], f[2], f[3], gu, hi, lo, colpart, dbias)
    else:
        call("ab_softargmax3d_bwd_x3_bias", x, B, C, D, DP, H, W, f[1], f[2], f[3], gu, gc, hi, lo, colpart, dbias)
    return hi, lo, colpart, dbias


# ---------------------------------------------------------------- checks
TALLY = {"compared": 0, "repeat": 0, "bits": 0, "ratio": {}}


def close(section, what, got, ref, rtol, atol):
    """|got - ref| <= atol + rtol |ref| elementwise, in float64; keeps the largest error / tolerance of each section."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    ratio = float(((got - ref).abs() / (atol + rtol * ref.abs())).max()) if got.numel() else 0.0
    TALLY["compared"] += 1
    if ratio > TALLY["ratio"].get(section, (-1.0, ""))[0]:
        TALLY["ratio"][section] = (ratio, what)
    print(f"  {what}: err / tol = {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: err / tol = {ratio:.3f} (max err {float((got - ref).abs().max()):.3e})"


def same_bits(what, a, b):
    assert bits_equal(a, b), f"{what}: not bit-equal"
    TALLY["bits"] += 1


def check_forward(section, what, f, r, norm, core, conf_atol=1e-8):
    """conf_atol = 0 at small S: conf = max sigmoid(x) is ~2e-8 there, and an absolute 1e-8 would allow half of it.  The relative 3e-5
    alone still holds with room: conf = exp(m), m = log sigmoid(x) near -20 carries two fp32 roundings of half an ulp (2^-20 each, 1.9e-6
    relative in conf together) and the exponential a few 1e-7 more."""
    close(section, f"{what} uvd", f[1], r.uvd, 0.0, 3e-6)
    close(section, f"{what} conf", f[2], r.conf, 3e-5, conf_atol)
    if norm == 0:      # the softmax head's stat[..., 0] is the class maximum itself
        same_bits(f"{what} stat max", f[3][..., 0].cpu(), core.float().reshape(core.shape[0], core.shape[1], -1).amax(2))


def check_dlogits(section, what, dl, r, dt, C, D, DP, planes=False):
    got = from_nhwc(dl, C, DP)
    scale = float(r.grad.abs().max()) + 1e-300
    rtol, a = (2e-4, 2e-5) if planes else (1e-4, 1e-5) if dt == F32 else (1e-2, 1e-2)
    close(section, f"{what} dlogits", got[:, :, :D], r.grad, rtol, a * scale)
    assert float(got[:, :, D:].abs().sum()) == 0.0, f"{what}: a padded depth slot of dlogits is not 0"


def check_dbias(section, what, dbias, r, C, D, DP):
    got = dbias.detach().cpu().double().reshape(C, DP)
    ref = r.grad.sum(dim=(0, 3, 4))
    scale = float(r.grad.abs().sum(dim=(0, 3, 4)).max()) + 1e-300
    close(section, f"{what} dbias", got[:, :D], ref, 0.0, 2e-6 * scale)
    assert float(got[:, D:].abs().sum()) == 0.0, f"{what}: a padded depth slot of dbias is not 0"


def _id(case):
    return case[-1].replace(" ", "").replace(";", ",")


# ---------------------------------------------------------------- 1. stage 1 (+ stage 2) forward
@pytest.mark.parametrize("norm", (0, 1), ids=NORMS)
@pytest.mark.parametrize("dt", (F32, BF16))
@pytest.mark.parametrize("case", S1, ids=_id)
def test_stage1_forms(case, dt, norm):
    form, C, D, DP, B, H, W, what = case
    expect_form(form, 0, dt, C, D, DP, norm)
    o = operands(dt, C, D, DP, B, H, W)
    r = reference(dt, C, D, DP, B, H, W, norm, grad=False)
    x = nhwc(o.core, DP).cuda()
    f = twice(lambda: fwd(x, C, D, DP, norm))
    check_forward(1, f"form {form} {dt} {NORMS[norm]} [{what}]", f, r, norm, o.core)


# ---------------------------------------------------------------- 2. stage 2 alone
@pytest.mark.parametrize("case", S2, ids=lambda c: "x".join(map(str, c)))
def test_stage2_alone_is_bit_equal_to_the_forward(case):
    """ab_softargmax3d_stage2 (the entry the fused final layer feeds) on the part rows of a forward call: 1, 2 and 81 tiles."""
    C, D, DP, B, H, W = case
    x = nhwc(operands(F32, C, D, DP, B, H, W).core, DP).cuda()
    expect_form(restated_form(0, C, D, DP), 0, F32, C, D, DP, 0)
    part, uvd, conf, stat = twice(lambda: fwd(x, C, D, DP, 0))
    nt = ntiles(H, W)
    assert nt == -(-H * W // 64)

    def launch():
        o = nan(B, C, 3), nan(B, C), nan(B, C, 2)
        call("ab_softargmax3d_stage2", part, B, C, nt, *o)
        return o
    u2, c2, s2 = twice(launch)
    same_bits("stage2 uvd", u2, uvd), same_bits("stage2 conf", c2, conf), same_bits("stage2 stat", s2, stat)


# ---------------------------------------------------------------- 3. backward, dlogits in the logits' dtype
@pytest.mark.parametrize("v", VARIANTS)
@pytest.mark.parametrize("dt", (F32, BF16))
@pytest.mark.parametrize("case", BW, ids=_id)
def test_backward_forms(case, dt, v):
    form, C, D, DP, B, H, W, what = case
    norm, with_conf = variant(v)
    expect_form(form, 1, dt, C, D, DP, norm)
    o = operands(dt, C, D, DP, B, H, W)
    r = reference(dt, C, D, DP, B, H, W, norm, with_conf)
    x = nhwc(o.core, DP).cuda()
    expect_form(restated_form(0, C, D, DP), 0, dt, C, D, DP, norm)
    f = twice(lambda: fwd(x, C, D, DP, norm))
    gu, gc = o.g_uvd.cuda(), (o.g_conf.cuda() if with_conf else None)
    (dl,) = twice(lambda: bwd(x, C, D, DP, norm, f, gu, gc))
    tag = f"form {form} {dt} {v} [{what}]"
    check_dlogits(3, tag, dl, r, dt, C, D, DP)

    def inplace():
        xi = x.clone()
        return bwd(xi, C, D, DP, norm, f, gu, gc, dl=xi)
    same_bits(f"{tag} inplace", twice(inplace)[0], dl)


# ---------------------------------------------------------------- 4. backward, dlogits as split planes, with and without the bias gradient
@pytest.mark.parametrize("v", VARIANTS)
@pytest.mark.parametrize("case", SP, ids=_id)
def test_split_plane_forms(case, v):
    f2, f3, C, D, DP, B, H, W, what = case
    norm, with_conf = variant(v)
    expect_form(f2, 2, F32, C, D, DP, norm)
    expect_form(f3, 3, F32, C, D, DP, norm)
    o = operands(F32, C, D, DP, B, H, W)
    r = reference(F32, C, D, DP, B, H, W, norm, with_conf)
    x = nhwc(o.core, DP).cuda()
    expect_form(restated_form(0, C, D, DP), 0, F32, C, D, DP, norm)
    f = twice(lambda: fwd(x, C, D, DP, norm))
    gu, gc = o.g_uvd.cuda(), (o.g_conf.cuda() if with_conf else None)
    hi, lo = twice(lambda: bwd_split(x, C, D, DP, norm, f, gu, gc, False))
    bhi, blo, _, dbias = twice(lambda: bwd_split(x, C, D, DP, norm, f, gu, gc, True))
    tag = f"{v} [{what}]"
    same_bits(f"form {f3} vs {f2} {tag} hi", bhi, hi), same_bits(f"form {f3} vs {f2} {tag} lo", blo, lo)
    check_dlogits(4, f"form {f2} {tag}", hi.double() + lo.double(), r, F32, C, D, DP, planes=True)
    check_dbias(4, f"form {f3} {tag}", dbias, r, C, D, DP)


# ---------------------------------------------------------------- 5. the sigmoid head at small weight sums
@pytest.mark.parametrize("dt", (F32, BF16))
@pytest.mark.parametrize("case", SMALL_S, ids=_id)
def test_sigmoid_small_weight_sum(case, dt):
    """Logits around -20: S = sum sigmoid(x) is of the order of the reference's 1e-7, so uvd = sum(w coord) / (S + 1e-7) and its gradient
    w (1 - w) (coord - uvd) / (S + 1e-7) differ from the softmax constants 1 / (S (1 + 1e-7)) by tens of percent."""
    C, D, DP, B, H, W, what = case
    o = operands(dt, C, D, DP, B, H, W, small_s=True)
    r = reference(dt, C, D, DP, B, H, W, 1, small_s=True)
    x = nhwc(o.core, DP).cuda()
    expect_form(restated_form(0, C, D, DP), 0, dt, C, D, DP, 1)
    f = twice(lambda: fwd(x, C, D, DP, 1))
    tag = f"small S {dt} [{what}]"
    check_forward(5, tag, f, r, 1, o.core, conf_atol=0.0)
    gu = o.g_uvd.cuda()
    expect_form(restated_form(1, C, D, DP), 1, dt, C, D, DP, 1)
    (dl,) = twice(lambda: bwd(x, C, D, DP, 1, f, gu, None))
    check_dlogits(5, tag, dl, r, dt, C, D, DP)
    if dt == F32 and (C * DP) % 2 == 0:
        expect_form(restated_form(2, C, D, DP), 2, dt, C, D, DP, 1)
        expect_form(restated_form(3, C, D, DP), 3, dt, C, D, DP, 1)
        hi, lo = twice(lambda: bwd_split(x, C, D, DP, 1, f, gu, None, False))
        bhi, blo, _, dbias = twice(lambda: bwd_split(x, C, D, DP, 1, f, gu, None, True))
        same_bits(f"{tag} hi", bhi, hi), same_bits(f"{tag} lo", blo, lo)
        check_dlogits(5, f"{tag} planes", hi.double() + lo.double(), r, F32, C, D, DP, planes=True)
        check_dbias(5, tag, dbias, r, C, D, DP)


# ---------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: f"C{c[1]}-D{c[2]}-DP{c[3]}-gc{int(c[4])}-norm{c[5]}")
def test_refusals_leave_the_outputs_untouched(case):
    entries, C, D, DP, with_conf, norm, code = case
    B, H, W = 2, 3, 3
    n = B * H * W * C * max(D, DP)
    z = lambda *s: torch.zeros(s, device="cuda")           # noqa: E731
    gc = z(B, C) if with_conf else None
    for dt in (F32, BF16):
        x = torch.zeros(n, dtype=TD[dt], device="cuda")
        for e in entries:
            if not (with_conf and e == 1):                 # g_conf is an argument of the launcher, not of the dispatch
                assert witness(e, F32 if e >= 2 else dt, C, D, DP, norm) == code
        if 0 in entries:
            outs = nan(B * ntiles(H, W) * C * 8), nan(B, C, 3), nan(B, C), nan(B, C, 2)
            assert abi("ab_softargmax3d_fwd_norm", x, DTC(dt), B, C, D, DP, H, W, norm, *outs) == code
            if norm == 0:
                assert abi("ab_softargmax3d_fwd", x, DTC(dt), B, C, D, DP, H, W, *outs) == code
            assert all(bool(torch.isnan(t).all()) for t in outs)
        if 1 in entries:
            dl = nan(n, dtype=TD[dt])
            assert abi("ab_softargmax3d_bwd_norm", x, DTC(dt), B, C, D, DP, H, W, norm, z(B, C, 3), z(B, C), z(B, C, 2), z(B, C, 3), gc, dl) == code
            assert bool(torch.isnan(dl).all())
        if dt == F32 and 2 in entries:
            rows = abi("ab_softargmax3d_bwd_x3_bias_rows", B, H, W, stream=False)
            outs = nan(n, dtype=torch.bfloat16), nan(n, dtype=torch.bfloat16), nan(rows * C * max(D, DP)), nan(C * max(D, DP))
            stats = z(B, C, 3), z(B, C), z(B, C, 2), z(B, C, 3)
            assert abi("ab_softargmax3d_bwd_x3_norm", x, B, C, D, DP, H, W, norm, *stats, outs[0], outs[1], None, None) == code
            assert abi("ab_softargmax3d_bwd_x3_norm", x, B, C, D, DP, H, W, norm, *stats, *outs) == code
            if norm == 0:
                assert abi("ab_softargmax3d_bwd_x3", x, B, C, D, DP, H, W, *stats, None, outs[0], outs[1]) == code
                assert abi("ab_softargmax3d_bwd_x3_bias", x, B, C, D, DP, H, W, *stats, None, *outs) == code
            assert all(bool(torch.isnan(t).all()) for t in outs)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. guarded tails
TAIL = 4096


def guarded(shape, dtype=torch.float32):
    """A view of `shape` inside a byte buffer of 0xA5 with 4 KiB in front of it and 4 KiB behind it."""
    n = torch.empty((), dtype=dtype).element_size()
    for s in shape:
        n *= s
    buf = torch.full((TAIL + n + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[TAIL:TAIL + n].view(dtype).view(shape)


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
            assert bool((buf[:TAIL] == 0xA5).all()), f"{what}: wrote in front of its {name}"
            assert bool((buf[TAIL + n:] == 0xA5).all()), f"{what}: wrote behind its {name}"


# (forms of entries 0 .. 3 (None: refused, C*DP odd), C, D, DP, B, H, W)
GUARDED = (
    ((10, 20, None, None), 5, 9, 9, 3, 5, 13),              # the scalar family, C*DP = 45, 65 pixels
    ((121, 1628, 11628, 16428), 5, 9, 10, 3, 5, 13),        # pairs, C*DP = 50, DP > D
    ((160, 1628, 11628, 16428), 2, 257, 257, 1, 1, 3),      # pairs, D > 32 merge, 3 pixels
    ((181, 1628, 11644, 16444), 22, 28, 46, 1, 5, 13),      # KP = 8 and V = 4, C*DP = 1012
    ((121, 1628, 11628, 16428), 1, 2, 2, 3, 5, 13),         # C*DP = 2: the clamped loads
)


@pytest.mark.parametrize("case", GUARDED, ids=lambda c: "x".join(map(str, c[1:])))
def test_guarded_tails(case):
    """Every output of the forward, stage 2, both backwards and both split backwards inside a larger buffer of 0xA5, each launch twice into
    fresh guarded buffers; the results are the unguarded ones, bit for bit, and no byte around them changes."""
    forms, C, D, DP, B, H, W = case
    for dt in (F32, BF16):
        for norm in (0, 1):
            G = Guards()
            o = operands(dt, C, D, DP, B, H, W)
            x = nhwc(o.core, DP).cuda()
            gu = o.g_uvd.cuda()
            nt = ntiles(H, W)
            expect_form(forms[0], 0, dt, C, D, DP, norm)
            plain = twice(lambda: fwd(x, C, D, DP, norm))
            f = twice(lambda: fwd(x, C, D, DP, norm, out=(G.new("part", (B, nt, C, 8)), G.new("uvd", (B, C, 3)), G.new("conf", (B, C)), G.new("stat", (B, C, 2)))))
            for a, b, name in zip(f, plain, ("part", "uvd", "conf", "stat")):
                same_bits(f"guarded {name}", a[..., :5] if name == "part" else a, b[..., :5] if name == "part" else b)
            assert bool((_bytes(f[0][..., 5:]) == 0xA5).all()), "stage 1 wrote slots 5..7 of a part row"
            if norm == 0:
                def stage2():
                    s2 = G.new("uvd2", (B, C, 3)), G.new("conf2", (B, C)), G.new("stat2", (B, C, 2))
                    call("ab_softargmax3d_stage2", f[0], B, C, nt, *s2)
                    return s2
                s2 = twice(stage2)
                for a, b, name in zip(s2, plain[1:], ("uvd", "conf", "stat")):
                    same_bits(f"guarded stage2 {name}", a, b)
            expect_form(forms[1], 1, dt, C, D, DP, norm)
            (dl,) = twice(lambda: bwd(x, C, D, DP, norm, f, gu, None, dl=G.new("dlogits", tuple(x.shape), TD[dt])))
            same_bits("guarded dlogits", dl, twice(lambda: bwd(x, C, D, DP, norm, plain, gu, None))[0])
            if dt == F32 and forms[2] is not None:
                expect_form(forms[2], 2, dt, C, D, DP, norm)
                expect_form(forms[3], 3, dt, C, D, DP, norm)
                rows = B * -(-H * W // 64)
                planes = lambda k: (G.new("hi" + k, tuple(x.shape), torch.bfloat16), G.new("lo" + k, tuple(x.shape), torch.bfloat16))      # noqa: E731
                out = twice(lambda: bwd_split(x, C, D, DP, norm, f, gu, None, True,
                                              out=planes("") + (G.new("colpart", (rows, C * DP)), G.new("dbias", (C * DP,)))))
                ref = twice(lambda: bwd_split(x, C, D, DP, norm, plain, gu, None, True))
                for a, b, name in zip(out, ref, ("hi", "lo", "colpart", "dbias")):
                    same_bits(f"guarded bias-call {name}", a, b)
                out2 = twice(lambda: bwd_split(x, C, D, DP, norm, f, gu, None, False, out=planes("2")))
                same_bits("guarded hi", out2[0], ref[0]), same_bits("guarded lo", out2[1], ref[1])
            G.check(f"{dt} {NORMS[norm]} {case}")


def test_zz_report():
    """Prints what the docstring's "Observed" section records (run with -s)."""
    print(f"\ncomparisons against float64: {TALLY['compared']}; bit-equal comparisons: {TALLY['bits']}; repeated launches: {TALLY['repeat']}")
    for sec, (r, what) in sorted(TALLY["ratio"].items()):
        print(f"  section {sec}: largest err / tol = {r:.3f}  {what}")
