"""HoNet on the HIP kernels: the recovery kernels (ab_honet_recover_fwd / _bwd) against a float64 torch restatement and float64 autograd,
the whole model against the CPU torch module with the same weights (forward, one training step under ManoLoss + ObjLoss), determinism,
five eager TrainStep steps, checkpoints, refusals and the training script with the HoNet config."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
TRAIN_CFG = os.path.join(ROOT, "config", "ho3dv2_honet_mi355x.yaml")
FACTORS, SIZE, OFF_Z = (100.0, 0.0001), (160, 128), 0.4          # (trans, scale) factors; (width, height)
OUT = ("root_joint", "joints_3d_abs", "hand_verts_3d_abs", "joints_2d", "hand_verts_2d", "obj_center", "box_rot_rotmat", "obj_verts_3d_abs",
       "obj_verts_2d", "corners_3d_abs", "corners_2d", "corners_3d", "obj_verts_3d")


# ------------------------------------------------------------------------------------------------ the recovery kernels
def _chunk():
    from artiboost_amd import _lib
    nc = _lib.cdll().ab_honet_recover_chunks
    return next(n for n in range(1, 1 << 16) if nc(n + 1) == 2)


def _case(B, N, seed, zero_rot=False):
    """Seeded inputs (float32 CPU).  Sample 0: a 1e-3 rad rotation (exactly zero with zero_rot); the last sample: an off-centre principal
    point.  Scales keep both depths Z0 in 0.45 .. 1.0 m."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    u = lambda *s: torch.rand(*s, generator=g)       # noqa: E731
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = K[:, 1, 1] = 400.0 + 200.0 * u(B)
    K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = SIZE[0] / 2, SIZE[1] / 2, 1.0
    K[-1, 0, 2], K[-1, 1, 2] = SIZE[0] / 2 + 21.5, SIZE[1] / 2 - 13.25
    hand_st = torch.cat([1.0 + 9.0 * u(B, 1), 0.3 * r(B, 2)], 1)
    obj_st = torch.cat([1.0 + 9.0 * u(B, 1), 0.3 * r(B, 2), 0.8 * r(B, 3)], 1)
    a = r(3)
    obj_st[0, 3:] = 0.0 if zero_rot else 1e-3 * a / a.norm()
    return dict(hand_st=hand_st, obj_st=obj_st, cam_intr=K, joints_3d=0.05 * r(B, 21, 3), hand_verts_3d=0.05 * r(B, 778, 3),
                obj_verts_can=0.08 * r(B, N, 3), corners_can=0.08 * r(B, 8, 3))


def _ref64(c, corners, hand_st=None, obj_st=None):
    """The stage in float64 torch ops, from the model's definition (honet.HoNet: recover_3d_proj, hpregnet._rodrigues, K.p / depth)."""
    from artiboost_amd.honet import HoNet
    from artiboost_amd.hpregnet import _rodrigues, batch_persp_proj2d
    d = {k: v.double() for k, v in c.items()}
    hst = d["hand_st"] if hand_st is None else hand_st
    ost = d["obj_st"] if obj_st is None else obj_st
    K, B = d["cam_intr"], hst.shape[0]
    place = lambda pts, st: HoNet.recover_3d_proj(pts, K, st[:, :1].view(B, 1, 1) * FACTORS[1], st[:, 1:3].unsqueeze(1) * FACTORS[0],      # noqa: E731
                                                   input_res=SIZE, off_z=OFF_Z)
    j_abs, root = place(d["joints_3d"], hst)
    v_abs = d["hand_verts_3d"] + root
    R = _rodrigues(ost[:, 3:6])
    o_abs, centre = place(torch.einsum("bij,bnj->bni", R, d["obj_verts_can"]), ost)
    o = dict(root_joint=root, joints_3d_abs=j_abs, hand_verts_3d_abs=v_abs, joints_2d=batch_persp_proj2d(j_abs, K),
             hand_verts_2d=batch_persp_proj2d(v_abs, K), obj_center=centre, box_rot_rotmat=R, obj_verts_3d_abs=o_abs,
             obj_verts_2d=batch_persp_proj2d(o_abs, K), obj_verts_3d=o_abs - root)
    if corners:
        c_abs = torch.einsum("bij,bnj->bni", R, d["corners_can"]) + centre
        o.update(corners_3d_abs=c_abs, corners_2d=batch_persp_proj2d(c_abs, K), corners_3d=c_abs - root)
    return o


def _dev_args(c, corners, pitch):
    """Device tensors; pitch None: dense [B,3] / [B,6] head rows, else rows of a [B, pitch] buffer (the padded head outputs)."""
    dv = {k: v.cuda().contiguous() for k, v in c.items()}
    if pitch is not None:
        for k, w in (("hand_st", 3), ("obj_st", 6)):
            buf = torch.full((dv[k].shape[0], pitch), 7.0, device="cuda")
            buf[:, :w] = dv[k]
            dv[k] = buf[:, :w]
    return (dv["hand_st"], dv["obj_st"], dv["cam_intr"], dv["joints_3d"], dv["hand_verts_3d"], dv["obj_verts_can"],
            dv["corners_can"] if corners else None, FACTORS, SIZE)


def _sizes():
    return [1, 157, 300, _chunk() + 1]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("corners", [True, False])
@pytest.mark.parametrize("pitch", [8, None])
@pytest.mark.parametrize("zero_rot", [False, True])
def test_recover_forward_matches_float64(B, corners, pitch, zero_rot):
    from artiboost_amd import kernels as K
    assert _chunk() + 1 > 300 and K.HONET_FWD_OUT == OUT
    for N in _sizes():
        c = _case(B, N, seed=100 * B + N % 97, zero_rot=zero_rot)
        o = K.honet_recover_fwd(*_dev_args(c, corners, pitch), off_z=OFF_Z)
        ref = _ref64(c, corners)
        zmin = min(float(ref[k][..., 2].min()) for k in ref if k.endswith("_3d_abs"))
        assert zmin > 0.2
        tol2d = 2e-6 * float(c["cam_intr"][:, 0, 0].max()) / zmin          # a 3-D error of the bound, through focal / depth
        for k in OUT:
            if k not in ref:
                assert o[k] is None, k
                continue
            assert tuple(o[k].shape) == tuple(ref[k].shape), k
            err = (o[k].cpu().double() - ref[k]).abs().max().item()
            assert err <= (tol2d if k.endswith("_2d") else 2e-6), (B, N, k, err)
        if zero_rot:
            assert torch.equal(o["box_rot_rotmat"][0].cpu(), torch.eye(3))
        o2 = K.honet_recover_fwd(*_dev_args(c, corners, pitch), off_z=OFF_Z, want_rel_verts=False)
        assert o2["obj_verts_3d"] is None and torch.equal(o2["obj_verts_3d_abs"], o["obj_verts_3d_abs"])


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("corners", [True, False])
@pytest.mark.parametrize("pitch", [8, None])
def test_recover_backward_matches_float64_autograd_and_is_reproducible(B, corners, pitch):
    from artiboost_amd import kernels as K
    for N in _sizes():
        c = _case(B, N, seed=200 * B + N % 89)
        hst, ost = c["hand_st"].double().requires_grad_(True), c["obj_st"].double().requires_grad_(True)
        j64, v64 = c["joints_3d"].double().requires_grad_(True), c["hand_verts_3d"].double().requires_grad_(True)
        ref = _ref64(dict(c, joints_3d=j64, hand_verts_3d=v64), corners, hst, ost)
        g = torch.Generator().manual_seed(N)
        ups = {k: torch.randn(ref[k].shape, generator=g) for k in OUT if k in ref}
        for k in ups:                                   # pixel gradients of a pixel-sized loss
            if k.endswith("_2d"):
                ups[k] *= 1e-3
        args = _dev_args(c, corners, pitch)
        for sel in [list(ups)] + [[k] for k in ups]:
            rg = torch.autograd.grad([ref[k] for k in sel], [hst, ost, j64, v64], [ups[k].double() for k in sel], retain_graph=True,
                                     allow_unused=True)
            rg = [torch.zeros_like(t) if r is None else r for r, t in zip(rg, (hst, ost, j64, v64))]
            grads = {k: ups[k].cuda() for k in sel}
            got = K.honet_recover_bwd(*args, grads, off_z=OFF_Z)
            for name, ours, r in zip(("g_hand_st", "g_obj_st", "g_joints_3d", "g_hand_verts_3d"), got, rg):
                err = (ours.cpu().double() - r).abs().max().item()
                assert err <= 1e-4 * r.abs().max().item(), (B, N, sel, name, err, r.abs().max().item())
            if len(sel) > 1:
                again = K.honet_recover_bwd(*args, grads, off_z=OFF_Z)
                assert all(torch.equal(a, b) for a, b in zip(got, again))
            else:                                       # NULL gradient pointers == explicit zeros, bit for bit
                zeros = {k: (ups[k].cuda() if k in sel else torch.zeros_like(ups[k]).cuda()) for k in ups}
                full = K.honet_recover_bwd(*args, zeros, off_z=OFF_Z)
                assert all(torch.equal(a, b) for a, b in zip(got, full)), (B, N, sel)
        if pitch is not None:                           # strided outputs: only the first 3 / 6 columns are written
            gh, go = torch.full((B, pitch), 5.0, device="cuda"), torch.full((B, pitch), 5.0, device="cuda")
            K.honet_recover_bwd(*args, {k: v.cuda() for k, v in ups.items()}, off_z=OFF_Z, g_hand_st=gh[:, :3], g_obj_st=go[:, :6])
            assert (gh[:, 3:] == 5.0).all() and (go[:, 6:] == 5.0).all()
            dense = K.honet_recover_bwd(*args, {k: v.cuda() for k, v in ups.items()}, off_z=OFF_Z)
            assert torch.equal(gh[:, :3], dense[0]) and torch.equal(go[:, :6], dense[1])


# ------------------------------------------------------------------------------------------------ the whole model
ARCH = {"TYPE": "HoNet", "PRETRAINED": "", "PREVIOUS": [], "OBJ_TRANS_FACTOR": 100, "OBJ_SCALE_FACTOR": 0.0001,
        "BACKBONE": {"TYPE": "ResNet18", "PRETRAINED": False, "FREEZE_BATCHNORM": False},
        "HEAD": {"TYPE": "ManoBranch", "MANO_ASSETS_ROOT": "assets/mano_v1_2", "INPUT_DIM": 512, "NCOMPS": 15, "USE_PCA": True, "USE_SHAPE": True}}
PRESET = {"IMAGE_SIZE": [128, 128], "HEATMAP_SIZE": [16, 16], "CENTER_IDX": 0}
CRIT = [{"TYPE": "ManoLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_HAND_VERTS_3D": 1.0, "LAMBDA_SHAPE_REG": 5.0e-7, "LAMBDA_POSE_REG": 5.0e-6},
        {"TYPE": "ObjLoss", "LAMBDA_OBJ_VERTS_3D": 1.0}]
LAMBDAS = [1.0, 1.0]
KEYS3D = ("joints_3d_abs", "corners_3d_abs", "hand_verts_3d_abs", "obj_verts_3d_abs", "obj_verts_3d", "corners_3d", "root_joint", "obj_center")


def _batch(B, seed, N=300, corners=True):
    from gen_batch import make_batch
    b = make_batch(B, 128, seed)
    g = torch.Generator().manual_seed(seed + 1)
    b["obj_verts_can"] = 0.06 * torch.randn(B, N, 3, generator=g)
    b["obj_verts_3d"] = b["obj_verts_can"] + 0.05 * torch.randn(B, 1, 3, generator=g)
    b["hand_verts_3d"] = 0.05 * torch.randn(B, 778, 3, generator=g)
    if not corners:
        for k in ("corners_3d", "corners_vis"):
            del b[k]
    return b


def _models(dtype):
    """(CPU torch HoNet with settled BatchNorm statistics, device HoNet holding the same state)."""
    import artiboost_amd.honet  # noqa: F401  (registers HoNet)
    from artiboost_amd import registry as R
    from artiboost_amd.regnet import HoNetHIP
    torch.manual_seed(0)
    cpu = R.build_arch_model_list(ARCH, preset_cfg=PRESET)[0]
    with torch.no_grad():
        bns = [m for m in cpu.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        for m in bns:
            m.momentum = None
            m.reset_running_stats()
        cpu.train()
        cpu(_batch(8, 1))
        for m in bns:
            m.momentum = 0.1
    dev = R.build_arch_model_list(dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE=dtype), preset_cfg=PRESET)[0]
    assert isinstance(dev, HoNetHIP)
    dev.load_state_dict(cpu.state_dict())
    return cpu, dev


@pytest.mark.parametrize("dtype,tol", [("f32", 2e-5), ("bf16x3", 1e-3)])
def test_model_forward_matches_the_cpu_module(dtype, tol):
    cpu, dev = _models(dtype)
    for corners in (True, False):
        batch = _batch(4, 21, corners=corners)
        for train in (True, False):
            cpu.train(train); dev.train(train)
            with torch.no_grad():
                ref, out = cpu(batch), dev(batch)
            assert set(out) == set(ref)
            assert {k for k, v in out.items() if v is None} == {k for k, v in ref.items() if v is None} == (set() if corners else {"corners_3d_abs", "corners_2d", "corners_3d"})
            for k, v in ref.items():
                if v is not None:
                    assert tuple(out[k].shape) == tuple(v.shape), k
            for k in KEYS3D:
                if ref[k] is not None:
                    err = (out[k].cpu() - ref[k]).abs().max().item()
                    assert err <= tol, (train, k, err)
    # checkpoints: HIP -> CPU module -> HIP with equal outputs, under the CPU module's key set
    sd = dev.state_dict()
    assert set(sd) == set(cpu.state_dict())
    cpu.load_state_dict(sd, strict=True)
    import artiboost_amd.registry as R
    dev2 = R.build_arch_model_list(dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE=dtype), preset_cfg=PRESET)[0]
    dev2.load_state_dict(cpu.state_dict(), strict=True)
    dev.eval(); dev2.eval()
    with torch.no_grad():
        a, b = dev(batch), dev2(batch)
    assert all(torch.equal(a[k], b[k]) for k in a if a[k] is not None)
    assert dev.CHECKPOINT_NAME == "HoNet"


def test_refusals():
    import artiboost_amd.honet  # noqa: F401
    from artiboost_amd import registry as R
    with pytest.raises(NotImplementedError, match="FUSED_STEP"):
        R.build_arch_model_list(dict(ARCH, DEVICE="cuda", FUSED_STEP=True), preset_cfg=PRESET)
    with pytest.raises(NotImplementedError, match="MANO_FHB_ADAPTOR"):
        R.build_arch_model_list(dict(ARCH, DEVICE="cuda", MANO_FHB_ADAPTOR=True), preset_cfg=PRESET)
    with pytest.raises(NotImplementedError):
        R.build_arch_model_list(dict(ARCH, DEVICE="cuda", HEAD=dict(ARCH["HEAD"], USE_SHAPE=False)), preset_cfg=PRESET)
    with pytest.raises(NotImplementedError):
        R.build_arch_model_list(dict(ARCH, DEVICE="cuda", BACKBONE=dict(ARCH["BACKBONE"], TYPE="ResNet50")), preset_cfg=PRESET)
    dev = R.build_arch_model_list(dict(ARCH, DEVICE="cuda"), preset_cfg=PRESET)[0]
    with pytest.raises(RuntimeError, match="DataParallel"):
        dev._replicate_for_data_parallel()
    with pytest.raises(ValueError, match="IMAGE_SIZE"):
        dev(dict(_batch(2, 3), image=torch.zeros(2, 3, 64, 64)))


# the bounds test_gpu_regnet.py::test_training_step_gradient_matches_cpu_autograd holds HOPRegNet to (same trunk, same head kernels)
GRAD_TOL = {"f32": dict(heads=5e-3, g_mean=5e-3, trunk_tensor=3e-2, whole=3e-2),
            "bf16x3": dict(heads=2e-2, g_mean=2e-2, trunk_tensor=6e-2, whole=3e-2)}


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_training_step_gradient_matches_cpu_autograd(dtype):
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    tol = GRAD_TOL[dtype]
    cpu, dev = _models(dtype)
    crit = lambda: Criterion({"LAMBDAS": LAMBDAS}, R.build_criterion_loss_list(CRIT, preset_cfg=PRESET, LAMBDAS=LAMBDAS))  # noqa: E731
    batch = _batch(4, 33)
    cpu.train(); dev.train()
    feats, orig = {}, cpu.base_net.forward

    def keep_mean(**kw):
        f = orig(**kw)
        f["res_layer4_mean"].retain_grad()
        feats.update(f)
        return f
    cpu.base_net.forward = keep_mean
    total_r, losses_r = crit().compute_losses(cpu(batch), batch)
    assert losses_r["hand_verts_3d_loss"] is not None and losses_r["obj_verts_3d_loss"] is not None
    total_r.backward()
    seen, net_bwd = {}, dev.net.backward

    def keep_g_mean(*a, **kw):
        seen["g_mean"] = kw["g_mean"].clone()
        return net_bwd(*a, **kw)
    dev.net.backward = keep_g_mean
    total, _ = crit().compute_losses(dev(batch), batch)
    total.backward()
    assert dev.flat_param.grad is dev.store.grad
    np.testing.assert_allclose(float(total.detach()), float(total_r.detach()), rtol=1e-4 if dtype == "f32" else 1e-2)
    rel = lambda a, b: (a.cpu() - b).norm().item() / max(b.norm().item(), 1e-30)      # noqa: E731
    e_mean = rel(seen["g_mean"], feats["res_layer4_mean"].grad)
    grads = dev.store.reference_state_dict(grads=True)
    ref = {k: p.grad for k, p in cpu.named_parameters() if p.grad is not None}
    assert set(ref) <= set(grads)
    errs = {k: rel(grads[k], r) for k, r in ref.items()}
    heads = {k: e for k, e in errs.items() if not k.startswith("base_net.")}
    trunk = {k: e for k, e in errs.items() if k.startswith("base_net.")}
    whole = rel(torch.cat([grads[k].flatten() for k in ref]), torch.cat([r.flatten() for r in ref.values()]))
    print(f"\n{dtype}: heads {max(heads.values()):.2e}, g_mean {e_mean:.2e}, trunk tensor max {max(trunk.values()):.2e}, whole {whole:.2e}")
    assert e_mean <= tol["g_mean"], e_mean
    assert len(heads) == 16 and {k.split(".")[0] for k in heads} == {"mano_branch", "mano_transhead", "obj_transhead"}
    assert max(heads.values()) <= tol["heads"], sorted(heads.items(), key=lambda kv: -kv[1])[:3]
    assert max(trunk.values()) <= tol["trunk_tensor"], sorted(trunk.items(), key=lambda kv: -kv[1])[:3]
    assert whole <= tol["whole"], whole


def test_hip_backward_is_deterministic():
    _, dev = _models("bf16x3")
    batch = _batch(4, 5)
    dev.train()
    g = torch.Generator().manual_seed(3)
    ups, grads = None, []
    for _ in range(2):
        out = dev(batch)
        ts = [v for k, v in sorted(out.items()) if v is not None and v.requires_grad]
        assert len(ts) >= 20
        if ups is None:
            ups = [torch.randn(t.shape, generator=g).cuda() for t in ts]
        torch.autograd.backward(ts, ups)
        torch.cuda.synchronize()
        grads.append(dev.store.grad.clone())
    assert grads[0].abs().sum() > 0 and torch.equal(grads[0], grads[1])


def test_train_step_reduces_the_loss_on_a_fixed_batch():
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    from artiboost_amd.models import Arch
    from artiboost_amd.netutils import build_optimizer
    from artiboost_amd.optim import FusedClipAdam
    from artiboost_amd.train import TrainStep
    import artiboost_amd.honet  # noqa: F401
    arch = dict(ARCH, DEVICE="cuda")
    model = Arch({"ARCH": arch}, R.build_arch_model_list(arch, preset_cfg=PRESET))
    crit = Criterion({"LAMBDAS": LAMBDAS}, R.build_criterion_loss_list(CRIT, preset_cfg=PRESET, LAMBDAS=LAMBDAS))
    opt = build_optimizer(model.models_params, OPTIMIZER="adam", LR=3e-4, WEIGHT_DECAY=0)
    assert isinstance(opt, FusedClipAdam)
    opt.max_norm = 1.0
    batch = {k: v.cuda() for k, v in _batch(4, 8).items()}
    ts = TrainStep(model, crit, opt, batch, use_graph=True)
    assert ts.fused is None and not ts.use_graph and ts.model_key == "HoNet"
    vals = []
    for _ in range(5):
        _, total, losses = ts()
        vals.append(float(total.detach()))
    assert np.isfinite(vals).all() and vals[-1] < vals[0], vals


def test_loader_epoch_batches_with_and_without_mesh_queries():
    """A real synthetic epoch: MANAGER.MESH_QUERIES adds three entries to the eager batches and changes nothing else; the added entries
    agree with the batch's own ground truth (MANO's finger-tip joints ARE vertices; the object's corners obey the same transform)."""
    import yaml
    from artiboost_amd.assets import SceneAssets
    from artiboost_amd.hpregnet import MANO_JOINT_REORDER, MANO_TIPS
    from artiboost_amd.synth import ArtiBoostLoader
    cfg = yaml.safe_load(open(TRAIN_CFG))
    preset = dict(cfg["DATA_PRESET"], IMAGE_SIZE=[64, 64])
    assets = SceneAssets("HO3D", seed=1)
    n = cfg["MANAGER"]["MESH_QUERIES"]
    first = {}
    for tag, mgr in (("on", cfg["MANAGER"]), ("off", {k: v for k, v in cfg["MANAGER"].items() if k != "MESH_QUERIES"})):
        ld = ArtiBoostLoader.from_assets(assets, mgr, preset, 6, 12, compute_dtype=torch.float32, random_seed=5)
        ld.prepare()
        first[tag] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in next(iter(ld)).items()}
    on, off = first["on"], first["off"]
    assert set(on) - set(off) == {"obj_verts_can", "obj_verts_3d", "hand_verts_3d"} and set(off) <= set(on)
    for k, v in off.items():
        assert torch.equal(on[k], v) if torch.is_tensor(v) else on[k] == v, k
    assert on["obj_verts_can"].shape == (6, n, 3) == on["obj_verts_3d"].shape and on["hand_verts_3d"].shape == (6, 778, 3)
    tips = [MANO_JOINT_REORDER.index(16 + i) for i in range(5)]
    err = (on["hand_verts_3d"][:, MANO_TIPS] - on["joints_3d"][:, tips]).abs().max().item()
    assert err <= 2e-6, err                       # the 3-D fp32 bound of this file: two 3x3 products and a subtraction at ~0.6 m
    T, root = on["obj_transf"], on["root_joint"]
    want = torch.einsum("bij,bnj->bni", T[:, :3, :3], on["obj_verts_can"]) + T[:, None, :3, 3] - root[:, None]
    assert (on["obj_verts_3d"] - want).abs().max().item() <= 2e-6
    # the canonical vertices lie inside the sample's canonical box, whose posed corners are the batch's corners_3d
    lo, hi = on["corners_can"].min(1).values, on["corners_can"].max(1).values
    assert ((on["obj_verts_can"] >= lo[:, None] - 1e-6) & (on["obj_verts_can"] <= hi[:, None] + 1e-6)).all()


def test_train_script_with_the_honet_config(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(TRAIN_CFG))
    cfg["TRAIN"]["EPOCH"] = 1
    y = tmp_path / "cfg.yaml"
    y.write_text(yaml.dump(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "train", "train_artiboost.py"), "--cfg", str(y), "--gpu_id", "0", "--gpu_render_id", "0",
           "--batch_size", "8", "--exp_id", "t", "--snapshot", "1", "--synth_len", "16", "--size", "64"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 1 and "final_loss" in lines[-1]          # one epoch of 16 / 8 = two steps
    exp = [d for d in os.listdir(tmp_path / "exp") if d.startswith("t_")]
    ck = tmp_path / "exp" / exp[0] / "checkpoints" / "checkpoint"
    sd = torch.load(ck / "HoNet.pth.tar", map_location="cpu", weights_only=False)
    assert "obj_transhead.final_layer.weight" in sd and "mano_transhead.decoder.0.bias" in sd and any(k.startswith("base_net.") for k in sd)
