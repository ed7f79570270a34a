"""HOPRegNet's device step, stage by stage, against torch on the CPU in float64 built from the same state dict:

  heads      the regression heads alone (trunk and MANO stubbed out): outputs, the 12 head gradients and the gradient reaching
             res_layer4_mean, held to the fp32 dot-product bound propagated through the layers; padding rows of the head weights
  bridge     heads + the MANO backward, every upstream gradient live; the None paths of _backward
  trunk      HybridNet's backward from a fixed gradient of res_layer4_mean, with frozen and with training-mode BatchNorm (the latter
             against the noise floor of CPU fp32 autograd)
  forward    all 18 output keys of the whole model, train and eval mode

test_gpu_regnet.py checks the same model end to end against fp32 CPU autograd; these tests locate an error in one stage."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

U = 2.0 ** -24          # fp32 unit roundoff
HEAD_KEYS = ("mano_branch.base_layer.0", "mano_branch.base_layer.2", "mano_branch.pose_reg", "mano_branch.shape_reg.0",
             "obj_transfhead.decoder.0", "obj_transfhead.final_layer")
ARCH = {"TYPE": "HOPRegNet", "PRETRAINED": "", "PREVIOUS": [],
        "BACKBONE": {"TYPE": "ResNet34", "PRETRAINED": False, "FREEZE_BATCHNORM": False},
        "HEAD": {"TYPE": "ManoBranch", "MANO_ASSETS_ROOT": "assets/mano_v1_2", "INPUT_DIM": 512, "NCOMPS": 15, "USE_PCA": True, "USE_SHAPE": True}}


def _pair(dtype="f32", size=64, ncomps=15, center=0, frozen=False, sd_edit=None):
    """(CPU torch HOPRegNet, device HOPRegNet) holding the same state; sd_edit(state_dict) may change the state first."""
    import artiboost_amd.hpregnet  # noqa: F401  (registers HOPRegNet)
    from artiboost_amd import registry as R
    preset = {"IMAGE_SIZE": [size, size], "HEATMAP_SIZE": [28, 28], "CENTER_IDX": center}
    head = dict(ARCH["HEAD"], NCOMPS=ncomps)
    torch.manual_seed(ncomps + 100 * center)
    cpu = R.build_arch_model_list(dict(ARCH, HEAD=head), preset_cfg=preset)[0]
    if sd_edit is not None:
        sd = cpu.state_dict()
        sd_edit(sd)
        cpu.load_state_dict(sd)
    bb = dict(ARCH["BACKBONE"], FREEZE_BATCHNORM=frozen)
    dev = R.build_arch_model_list(dict(ARCH, HEAD=head, BACKBONE=bb, DEVICE="cuda", COMPUTE_DTYPE=dtype), preset_cfg=preset)[0]
    sd = cpu.state_dict()
    if frozen:          # FrozenBatchNorm2d keeps no counter
        sd = {k: v for k, v in sd.items() if not (k.startswith("base_net.") and k.endswith("num_batches_tracked"))}
    dev.load_state_dict(sd)
    dev.train()
    dev.net.pack_weights()
    return cpu, dev


# ------------------------------------------------------------------------------------------------ heads, float64 with error bounds
def _fmean(B, seed):
    """A res_layer4_mean stand-in: non-negative, exact zeros, some all-zero columns and (B > 1) one all-zero row."""
    g = torch.Generator().manual_seed(seed)
    f = 0.5 * torch.relu(torch.randn(B, 512, generator=g))
    f[:, ::9] = 0.0
    if B > 1:
        f[B // 2] = 0.0
    return f


def _heads_reference(cpu, fm, ups, mano_err=(0.0, 0.0)):
    """Float64 autograd of cpu's heads (+ its MANO layer) at res_layer4_mean = fm, and an elementwise bound of the device's error.

    ups: upstream gradients (pose, shape, verts, joints, full, transf), None = no gradient.  The bound is the first-order fp32 bound
    propagated through the layers: a linear layer adds (R + 2) u sum|a||b| for a reduction of length R (plus its bias and the final
    rounding) to |W| times the error of its input; ReLU does not increase it; a sum of two gradients adds u |sum|.  mano_err: a
    uniform error of the MANO backward's (pose, shape) gradient."""
    mb, th = copy.deepcopy(cpu.mano_branch).double(), copy.deepcopy(cpu.obj_transfhead).double()
    fm = fm.double().requires_grad_(True)
    h = mb.base_layer(fm)
    pose, shape = mb.pose_reg(h), mb.shape_reg(h)
    verts, joints, full = mb.mano_layer(pose, shape)
    transf = th(fm)
    outs = (pose, shape, verts, joints, full, transf)
    pairs = [(o, u.double()) for o, u in zip(outs, ups) if u is not None]
    params = {f"{n}.{k}": m.weight if k == "weight" else m.bias for n, m in
              (("mano_branch.base_layer.0", mb.base_layer[0]), ("mano_branch.base_layer.2", mb.base_layer[2]),
               ("mano_branch.pose_reg", mb.pose_reg), ("mano_branch.shape_reg.0", mb.shape_reg[0]),
               ("obj_transfhead.decoder.0", th.decoder[0]), ("obj_transfhead.final_layer", th.final_layer)) for k in ("weight", "bias")}
    gs = torch.autograd.grad([o for o, _ in pairs], [fm] + list(params.values()), [u for _, u in pairs], retain_graph=True)
    ref = dict(zip(["g_mean"] + list(params), gs))
    ref.update(zip(("pose", "shape", "verts", "joints", "full", "transf"), (o.detach() for o in outs)))
    # the gradient the heads receive: d/d(pose, shape) of everything downstream (direct + through MANO)
    gp, gsh = torch.autograd.grad([o for o, _ in pairs], [pose, shape], [u for _, u in pairs], allow_unused=True)
    gp = torch.zeros_like(pose) if gp is None else gp
    gsh = torch.zeros_like(shape) if gsh is None else gsh
    gt = ups[5].double() if ups[5] is not None else torch.zeros_like(transf)

    W = {n: params[n + ".weight"].detach() for n in HEAD_KEYS}
    b = {n: params[n + ".bias"].detach() for n in HEAD_KEYS}
    A = {n: W[n].abs() for n in HEAD_KEYS}
    x0 = fm.detach()

    def fwd(x, ex, n):
        z = x @ W[n].T + b[n]
        return z, ex @ A[n].T + (W[n].shape[1] + 2) * U * (x.abs() @ A[n].T + b[n].abs())

    def dgrad(g, eg, n, mask):
        R = -(-W[n].shape[0] // 8) * 8           # the device reduces over the padded width (zero rows)
        return (g @ W[n]) * mask, (eg @ A[n] + (R + 2) * U * (g.abs() @ A[n])) * mask

    def wgrad(g, eg, x, ex, n, err):
        M = g.shape[0]
        err[n + ".weight"] = (M + 2) * U * (g.abs().T @ x.abs()) + eg.T @ x.abs() + g.abs().T @ ex
        err[n + ".bias"] = (M + 2) * U * g.abs().sum(0) + eg.sum(0)

    err = {}
    z1, e1 = fwd(x0, torch.zeros_like(x0), HEAD_KEYS[0])
    h1, m1 = torch.relu(z1), (z1 > 0).double()
    z2, e2 = fwd(h1, e1, HEAD_KEYS[1])
    h2, m2 = torch.relu(z2), (z2 > 0).double()
    _, err["pose"] = fwd(h2, e2, HEAD_KEYS[2])
    _, err["shape"] = fwd(h2, e2, HEAD_KEYS[3])
    zd, ed = fwd(x0, torch.zeros_like(x0), HEAD_KEYS[4])
    d1, md = torch.relu(zd), (zd > 0).double()
    _, err["transf"] = fwd(d1, ed, HEAD_KEYS[5])
    egp = mano_err[0] + 2 * U * gp.abs()          # (the MANO part + the direct part, one fp32 addition)
    egs = mano_err[1] + 2 * U * gsh.abs()
    wgrad(gp, egp, h2, e2, HEAD_KEYS[2], err)
    wgrad(gsh, egs, h2, e2, HEAD_KEYS[3], err)
    ga, ea = dgrad(gp, egp, HEAD_KEYS[2], m2)
    gb, eb = dgrad(gsh, egs, HEAD_KEYS[3], m2)
    gh2, eh2 = ga + gb, ea + eb + U * (ga + gb).abs()
    wgrad(gh2, eh2, h1, e1, HEAD_KEYS[1], err)
    gh1, eh1 = dgrad(gh2, eh2, HEAD_KEYS[1], m1)
    wgrad(gh1, eh1, x0, 0 * x0, HEAD_KEYS[0], err)
    wgrad(gt, 0 * gt, d1, ed, HEAD_KEYS[5], err)
    gd1, egd1 = dgrad(gt, 0 * gt, HEAD_KEYS[5], md)
    wgrad(gd1, egd1, x0, 0 * x0, HEAD_KEYS[4], err)
    ga, ea = dgrad(gh1, eh1, HEAD_KEYS[0], 1.0)
    gb, eb = dgrad(gd1, egd1, HEAD_KEYS[4], 1.0)
    err["g_mean"] = ea + eb + U * (ga + gb).abs()
    assert torch.allclose(ga + gb, ref["g_mean"], rtol=1e-12, atol=1e-14)      # the bound's own chain is the reference's
    return ref, err


def _run_heads(dev, fm, ups):
    """dev._run + dev._backward with the trunk stubbed: -> (six outputs, g_mean the trunk would receive)."""
    seen = {}
    fmd = fm.cuda()
    dev.net.forward = lambda image=None, xpad=None: fmd                       # noqa: E731
    dev.net.backward = lambda g_mean=None, **kw: seen.update(g_mean=g_mean.clone())  # noqa: E731
    outs = dev._run(None, None, save=True)
    dev._backward(*[None if u is None else u.cuda() for u in ups])
    torch.cuda.synchronize()
    return [o.cpu() for o in outs], seen["g_mean"].cpu()


def _check_bound(name, got, ref, err, errs):
    d = (got.double() - ref).abs()
    errs[name] = float(d.max() / max(float(ref.abs().max()), 1e-30))
    bad = d > err
    assert not bad.any(), (name, int(bad.sum()), float(d.max()), float((d - err).max()))


def _check_padding(dev):
    """The padding rows of every head (output width rounded up to REG_PAD) hold zero weights and receive zero gradient, bit for bit."""
    p = dev.store
    live = 0
    for n in HEAD_KEYS:
        ew, eb = p.entries[n + ".weight"], p.entries[n + ".bias"]
        o = ew.ref_shape[0]
        gw, gb = p.gview(n + ".weight").view(ew.kshape[0], -1), p.gview(n + ".bias")
        w, bb = p.view(n + ".weight").view(ew.kshape[0], -1), p.view(n + ".bias")
        assert gw.shape[0] == eb.kshape[0] and gw.shape[0] % p.REG_PAD == 0
        if gw.shape[0] > o:
            live += 1
            for t in (gw, gb, w, bb):
                assert torch.count_nonzero(t[o:]).item() == 0, n
    return live


HEAD_CASES = [(nc, c, B) for nc in (15, 45) for c in (0, 9) for B in (1, 5, 37, 64)]


@pytest.mark.parametrize("ncomps,center,B", HEAD_CASES)
def test_heads_alone_match_float64_within_the_fp32_bound(ncomps, center, B):
    """Trunk and MANO out of the picture: res_layer4_mean is given, gradients arrive only on mano_pca_pose, mano_shape and transf
    (g_verts / g_joints zero, g_full None).  Outputs, the 12 head gradients and g_mean within the propagated fp32 bound; the padding
    rows stay exactly zero through two FusedClipAdam steps."""
    from artiboost_amd.optim import FusedClipAdam
    cpu, dev = _pair(ncomps=ncomps, center=center)
    fm = _fmean(B, seed=B + ncomps)
    g = torch.Generator().manual_seed(B * 3 + center)
    P = 3 + ncomps
    ups = [torch.randn(B, P, generator=g), torch.randn(B, 10, generator=g), torch.zeros(B, 778, 3), torch.zeros(B, 21, 3), None,
           torch.randn(B, 9, generator=g)]
    outs, g_mean = _run_heads(dev, fm, ups)
    ref, err = _heads_reference(cpu, fm, [ups[0], ups[1], None, None, None, ups[5]])
    errs = {}
    for k, o in zip(("pose", "shape", "transf"), (outs[0], outs[1], outs[5])):
        _check_bound(k, o, ref[k], err[k], errs)
    _check_bound("g_mean", g_mean, ref["g_mean"], err["g_mean"], errs)
    grads = {k: v.cpu() for k, v in dev.store.reference_state_dict(grads=True).items()}
    head_grads = [k for k in grads if not k.startswith("base_net.")]
    assert len(head_grads) == 12
    for k in head_grads:
        _check_bound(k, grads[k], ref[k], err[k], errs)
    # MANO on the device's own pose / shape: the bound of its forward test (test_gpu_regnet.py)
    v, j, full = copy.deepcopy(cpu.mano_branch.mano_layer).double()(outs[0].double(), outs[1].double())
    for o, r, tol in ((outs[2], v, 2e-6), (outs[3], j, 2e-6), (outs[4], full, 1e-6)):
        assert (o.double() - r).abs().max().item() <= tol
    print(f"\nheads ncomps={ncomps} center={center} B={B}: max error / max|ref| = {max(errs.values()):.2e} "
          f"({max(errs, key=errs.get)})")
    # padding rows: zero gradient, and zero weights after two optimizer steps
    assert _check_padding(dev) == (2 if ncomps == 45 else 3)
    opt = FusedClipAdam([dev.flat_param], lr=1e-2, model=dev)
    w0 = dev.store.view("mano_branch.pose_reg.weight").clone()
    for _ in range(2):
        dev.flat_param.grad = dev.store.grad
        opt.step()
        dev.net.pack_weights()
        _run_heads(dev, fm, ups)
        _check_padding(dev)
    assert not torch.equal(w0, dev.store.view("mano_branch.pose_reg.weight"))


@pytest.mark.parametrize("ncomps,center,B", [(15, 0, 37), (45, 9, 5), (15, 9, 64), (45, 0, 1)])
def test_heads_and_mano_bridge_match_float64(ncomps, center, B):
    """All six upstream gradients live: the MANO backward (held to 1e-4 of its scale by its own test) feeds the heads; that error is
    carried through the head bound.  g_verts, g_joints and g_full set to None, each in turn, give the same bits as zeros."""
    cpu, dev = _pair(ncomps=ncomps, center=center)
    fm = _fmean(B, seed=7 * B + ncomps)
    g = torch.Generator().manual_seed(B + 11 * center + ncomps)
    P = 3 + ncomps
    ups = [torch.randn(B, P, generator=g), torch.randn(B, 10, generator=g), torch.randn(B, 778, 3, generator=g),
           torch.randn(B, 21, 3, generator=g), torch.randn(B, 48, generator=g), torch.randn(B, 9, generator=g)]
    outs, g_mean = _run_heads(dev, fm, ups)
    # the MANO part of the pose / shape gradient, to scale its error
    mb = copy.deepcopy(cpu.mano_branch).double()
    pose, shape = outs[0].double().requires_grad_(True), outs[1].double().requires_grad_(True)
    gpc, gb = torch.autograd.grad(mb.mano_layer(pose, shape), [pose, shape], [u.double() for u in ups[2:5]])
    ref, err = _heads_reference(cpu, fm, ups, mano_err=(1e-4 * float(gpc.abs().max()), 1e-4 * float(gb.abs().max())))
    errs = {}
    for k, o in zip(("pose", "shape", "transf"), (outs[0], outs[1], outs[5])):
        _check_bound(k, o, ref[k], err[k], errs)
    _check_bound("g_mean", g_mean, ref["g_mean"], err["g_mean"], errs)
    grads = {k: v.cpu() for k, v in dev.store.reference_state_dict(grads=True).items()}
    for k in grads:
        if not k.startswith("base_net."):
            _check_bound(k, grads[k], ref[k], err[k], errs)
    print(f"\nbridge ncomps={ncomps} center={center} B={B}: max error / max|ref| = {max(errs.values()):.2e} "
          f"({max(errs, key=errs.get)})")
    assert _check_padding(dev) == (2 if ncomps == 45 else 3)
    g0 = dev.store.grad.clone()
    for i in (2, 3, 4):           # None == zeros, bit for bit
        zeros = [u if j != i else torch.zeros_like(u) for j, u in enumerate(ups)]
        nones = [u if j != i else None for j, u in enumerate(ups)]
        _, gm_z = _run_heads(dev, fm, zeros)
        gz = dev.store.grad.clone()
        _, gm_n = _run_heads(dev, fm, nones)
        assert torch.equal(gm_z, gm_n) and torch.equal(gz, dev.store.grad), i
        assert not torch.equal(gz, g0), i


# ------------------------------------------------------------------------------------------------ trunk backward from a fixed g_mean
def _bn_state(seed):
    """Non-trivial BatchNorm state of the trunk: running statistics (what a frozen BatchNorm applies) and affine parameters."""
    def edit(sd):
        g = torch.Generator().manual_seed(seed)
        for k in sd:
            if not k.startswith("base_net.") or not (".bn" in k or "downsample.1" in k):
                continue
            shp = sd[k].shape
            if k.endswith("running_mean"):
                sd[k] = 0.1 * torch.randn(shp, generator=g)
            elif k.endswith("running_var"):
                sd[k] = 0.5 + torch.rand(shp, generator=g)
            elif k.endswith("weight"):
                sd[k] = 0.5 + torch.rand(shp, generator=g)
            elif k.endswith("bias"):
                sd[k] = 0.1 * torch.randn(shp, generator=g)
    return edit


def _trunk_grads(net, image, G, train, fresh=True):
    """Autograd of res_layer4_mean.backward(G) through (fresh: a copy of) the torch trunk, in the dtype of `image`."""
    net = copy.deepcopy(net).to(image.dtype) if fresh else net
    net.train(train)
    fm = net(image=image)["res_layer4_mean"]
    fm.backward(G.to(image.dtype))
    return fm.detach(), {"base_net." + n: p.grad.double() for n, p in net.named_parameters() if p.grad is not None}


def _hip_trunk(dev, image, G):
    """-> (res_layer4_mean, reference-layout gradients, the forward's block records)."""
    dev.net.image_plane = "f32"
    fm = dev.net.forward(image=image.cuda())
    blocks = dev.net.saved["blocks"]
    dev.net.backward(g_mean=G.cuda())
    torch.cuda.synchronize()
    return fm.cpu(), {k: v.cpu() for k, v in dev.store.reference_state_dict(grads=True).items()}, blocks


def _device_masks_trunk(net, blocks):
    """A float64 copy of the torch trunk whose block ReLUs apply the device forward's own masks (a1 > 0, out > 0): the same
    function wherever both forwards agree on the sign of a pre-activation, and the linear map the device's backward computes where a
    rounding difference flipped one."""
    from artiboost_amd import kernels as K
    net = copy.deepcopy(net).double()

    def mask(t):
        v = t if (not isinstance(t, tuple) and t.dtype == torch.float32) else sum(p.float() for p in K._planes(t))
        return (v > 0).permute(0, 3, 1, 2).double().cpu()

    recs = {r["pre"][len("backbone."):]: r for r in blocks}
    for li in range(1, 5):
        for b, blk in enumerate(getattr(net, f"layer{li}")):
            r = recs[f"layer{li}.{b}"]
            m1, m2 = mask(r["a1"]), mask(r["out"])

            def fwd(x, blk=blk, m1=m1, m2=m2):
                out = blk.bn2(blk.conv2(blk.bn1(blk.conv1(x)) * m1))
                return (out + (x if blk.downsample is None else blk.downsample(x))) * m2
            blk.forward = fwd
    return net


def _rel(a, b):
    return (a.double() - b).norm().item() / max(b.norm().item(), 1e-30)


def _is_bn(k):
    return ".bn" in k or "downsample.1" in k


TRUNK_B, TRUNK_SIZE = 8, 128
# frozen BatchNorm, per-tensor relative error (L2) of the conv weight gradients against float64 through the device's ReLU masks: 3x the
# value measured on MI355X (f32 2.9e-6; bf16x3 7.0e-4 on the stem, whose ReLU / max-pool follow the reference's own masks, median 2e-5)
FROZEN_TOL = {"f32": 8.6e-6, "bf16x3": 2.0e-3}
# training-mode BatchNorm, bf16x3: whole-gradient / worst per-tensor relative error against float64, 3x the value measured on MI355X
# (2.2e-2 / 2.9e-2; CPU fp32 autograd: 8.5e-3 / 1.1e-2)
TRAIN_X3_TOL = (6.6e-2, 8.8e-2)


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_trunk_backward_with_frozen_batchnorm_matches_float64(dtype):
    """FREEZE_BATCHNORM: the trunk is a fixed piecewise-linear map, so its backward is held to float64 autograd through the device
    forward's own ReLU masks.  Against the plain float64 trunk the error is dominated by the few pre-activations whose sign the
    forward's rounding flipped (printed, not asserted)."""
    from gen_batch import make_batch
    cpu, dev = _pair(dtype, TRUNK_SIZE, frozen=True, sd_edit=_bn_state(5))
    image = make_batch(TRUNK_B, TRUNK_SIZE, 41)["image"]
    G = torch.randn(TRUNK_B, 512, generator=torch.Generator().manual_seed(3))
    fm, grads, blocks = _hip_trunk(dev, image, G)
    fm_plain, plain = _trunk_grads(cpu.base_net, image.double(), G, train=False)
    fm_ref, ref = _trunk_grads(_device_masks_trunk(cpu.base_net, blocks), image.double(), G, train=False, fresh=False)
    errs, errs_plain = {}, {}
    for k, r in ref.items():
        if _is_bn(k):
            assert torch.count_nonzero(grads[k]).item() == 0, k          # frozen: FrozenBatchNorm2d has no parameters to learn
        else:
            errs[k], errs_plain[k] = _rel(grads[k], r), _rel(grads[k], plain[k])
    assert len(errs) == 36
    worst = max(errs, key=errs.get)
    print(f"\ntrunk frozen {dtype}: res_layer4_mean {_rel(fm, fm_ref):.2e}; conv gradient per tensor, device masks: max {errs[worst]:.2e} "
          f"({worst}), median {float(np.median(list(errs.values()))):.2e}; plain float64: max {max(errs_plain.values()):.2e}, median "
          f"{float(np.median(list(errs_plain.values()))):.2e}")
    assert errs[worst] <= FROZEN_TOL[dtype], sorted(errs.items(), key=lambda kv: -kv[1])[:3]


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_trunk_backward_with_batch_statistics_against_the_cpu_fp32_floor(dtype):
    """Training-mode BatchNorm: the HIP trunk's gradient against float64, next to CPU fp32 autograd's own distance from float64 (the
    noise floor of fp32 arithmetic on this network).  f32: whole gradient within 3x the floor + 1e-4, each tensor within 10x its
    floor + 1e-4 (a single ReLU flip moves one tensor's value)."""
    from gen_batch import make_batch
    cpu, dev = _pair(dtype, TRUNK_SIZE, sd_edit=_bn_state(6))
    image = make_batch(TRUNK_B, TRUNK_SIZE, 43)["image"]
    G = torch.randn(TRUNK_B, 512, generator=torch.Generator().manual_seed(4))
    fm_ref, ref = _trunk_grads(cpu.base_net, image.double(), G, train=True)
    fm32, cpu32 = _trunk_grads(cpu.base_net, image.float(), G, train=True)
    fm, grads, _ = _hip_trunk(dev, image, G)
    keys = list(ref)
    assert len(keys) == 36 + 2 * 36
    cat = lambda d: torch.cat([d[k].double().flatten() for k in keys])      # noqa: E731
    whole_hip, whole_cpu = _rel(cat(grads), cat(ref)), _rel(cat(cpu32), cat(ref))
    per_hip = {k: _rel(grads[k], ref[k]) for k in keys}
    per_cpu = {k: _rel(cpu32[k], ref[k]) for k in keys}
    ratio = {k: per_hip[k] / (per_cpu[k] + 1e-12) for k in keys}
    worst = max(keys, key=lambda k: per_hip[k] - 10 * per_cpu[k])
    print(f"\ntrunk train {dtype}: res_layer4_mean HIP {_rel(fm, fm_ref):.2e} / CPU fp32 {_rel(fm32, fm_ref):.2e}; whole gradient HIP "
          f"{whole_hip:.2e} / CPU fp32 {whole_cpu:.2e}; per tensor max HIP {max(per_hip.values()):.2e} / CPU fp32 "
          f"{max(per_cpu.values()):.2e}, worst HIP/CPU ratio {max(ratio.values()):.1f} ({max(ratio, key=ratio.get)})")
    if dtype == "f32":
        assert whole_hip <= 3 * whole_cpu + 1e-4, (whole_hip, whole_cpu)
        assert per_hip[worst] <= 10 * per_cpu[worst] + 1e-4, (worst, per_hip[worst], per_cpu[worst])
    else:
        assert whole_hip <= TRAIN_X3_TOL[0], whole_hip
        assert max(per_hip.values()) <= TRAIN_X3_TOL[1], max(per_hip.items(), key=lambda kv: kv[1])


# ------------------------------------------------------------------------------------------------ whole-model forward, 18 keys
def _reference_outputs(model, batch):
    """The CPU module's forward in float64 (its object projection reads the canonical corners as fp32: restated here in float64)."""
    from artiboost_amd.hpregnet import batch_persp_proj2d, combine_outputs, mano_outputs
    from artiboost_amd.models import ortho6d_to_rotmat
    b = {k: v.double() if v.is_floating_point() else v for k, v in batch.items()}
    fm = model.base_net(image=b["image"])["res_layer4_mean"]
    t = model.obj_transfhead(fm)
    rot = ortho6d_to_rotmat(t[:, 3:]).view(-1, 3, 3)
    center = b["root_joint"] + t[:, :3]
    corners = rot.bmm(b["corners_can"].transpose(1, 2)).transpose(1, 2) + center.unsqueeze(1)
    obj = {"obj_center": center, "corners_3d_abs": corners, "obj_pred_tsl": t[:, :3], "obj_pred_rot": rot,
           "corners_2d": batch_persp_proj2d(corners, b["cam_intr"]), "box_rot_rotmat": rot, "boxroot_3d_abs": center}
    return combine_outputs(mano_outputs(model.mano_branch(fm), b, "cpu"), obj)


# max |HIP - float64| / max |float64| per key, over train and eval mode: 3x the value measured on MI355X (rounded down); root_joint is
# the batch's own tensor
FWD_TOL = {
    "f32": dict(mano_pca_pose=1.6e-5, mano_shape=2.0e-5, mano_full_pose=1.3e-5, hand_verts_3d=3.4e-6, joints_3d=3.4e-6,
                hand_verts_3d_abs=1.1e-6, joints_3d_abs=1.0e-6, hand_verts_2d=1.7e-6, joints_2d=1.3e-6, root_joint=0.0,
                obj_pred_tsl=5.6e-5, obj_pred_rot=4.3e-5, box_rot_rotmat=4.3e-5, obj_center=1.3e-5, boxroot_3d_abs=1.3e-5,
                corners_3d_abs=1.2e-5, corners_3d=3.5e-5, corners_2d=2.5e-5),
    "bf16x3": dict(mano_pca_pose=1.2e-4, mano_shape=2.4e-4, mano_full_pose=1.2e-4, hand_verts_3d=2.1e-5, joints_3d=2.0e-5,
                   hand_verts_3d_abs=7.1e-6, joints_3d_abs=6.8e-6, hand_verts_2d=8.9e-6, joints_2d=8.7e-6, root_joint=0.0,
                   obj_pred_tsl=4.8e-4, obj_pred_rot=8.7e-4, box_rot_rotmat=8.7e-4, obj_center=1.1e-4, boxroot_3d_abs=1.1e-4,
                   corners_3d_abs=2.5e-4, corners_3d=7.0e-4, corners_2d=4.1e-4)}


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_model_forward_all_keys_match_float64(dtype):
    from gen_batch import make_batch
    from test_gpu_regnet import _models
    cpu, dev = _models(dtype)
    m64 = copy.deepcopy(cpu).double()
    batch = make_batch(8, 224, 21)
    errs = {}
    for train in (True, False):
        m64.train(train); dev.train(train)
        with torch.no_grad():
            ref, out = _reference_outputs(m64, batch), dev(batch)
        assert set(out) == set(ref) == set(FWD_TOL[dtype]) and len(out) == 18
        for k in sorted(ref):
            errs[(train, k)] = (out[k].cpu().double() - ref[k]).abs().max().item() / max(ref[k].abs().max().item(), 1e-30)
    print(f"\nforward {dtype}: " + ", ".join(f"{'train' if t else 'eval'} {k} {e:.2e}" for (t, k), e in errs.items()))
    bad = {k: e for k, e in errs.items() if e > FWD_TOL[dtype][k[1]]}
    assert not bad, bad
