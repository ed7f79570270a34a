"""The fused criterion of the regression-based model (ab_reg_pose_loss / FusedRegCriterion) and HOPRegNet's graph-replayed training step
(ARCH.FUSED_STEP): the kernel against a float64 oracle, term by term; its loss dict against the registry losses; graph replay against
the eager route bit for bit, with a resumed checkpoint; the fused route's gradient against the autograd route's; training on a fixed
batch; the one-rank RCCL schedule; the training script with the shipped config; DeferredEpochMetrics against per-step feeding."""
import copy
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import learner_oracle as lo
from gen_batch import make_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_CFG = os.path.join(ROOT, "config", "ho3dv2_regbased_artiboost_mi355x_fused.yaml")

ARCH = {"TYPE": "HOPRegNet", "PRETRAINED": "", "PREVIOUS": [], "FUSED_STEP": True,
        "BACKBONE": {"TYPE": "ResNet34", "PRETRAINED": False, "FREEZE_BATCHNORM": False},
        "HEAD": {"TYPE": "ManoBranch", "MANO_ASSETS_ROOT": "assets/mano_v1_2", "INPUT_DIM": 512, "NCOMPS": 15, "USE_PCA": True, "USE_SHAPE": True}}
PRESET = {"IMAGE_SIZE": [224, 224], "HEATMAP_SIZE": [28, 28], "CENTER_IDX": 0}
# the shipped loss set (config/ho3dv2_regbased_artiboost_mi355x.yaml)
SHIPPED = dict(shape=5.0e-7, pose=5.0e-6, mano_j=0.0, j=1.0, c=0.2, jo=1.0, po=1.0, so=1.0, LAMBDAS=[1.0, 1.0, 0.1, 0.1])
ZERO = dict(shape=0.0, pose=0.0, mano_j=0.0, j=0.0, c=0.0, jo=0.0, po=0.0, so=0.0)
OWNER = dict(shape=0, pose=0, mano_j=0, j=1, c=1, jo=2, po=2, so=3)
# nine weight settings: the shipped one, and each of the eight terms alone (its lambda 1, its loss's LAMBDA 1, everything else 0)
SETTINGS = {"shipped": SHIPPED, **{t: dict(ZERO, **{t: 1.0}, LAMBDAS=[1.0 if i == OWNER[t] else 0.0 for i in range(4)]) for t in OWNER}}


def _criterion(w, preset=PRESET):
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    cfgc = [{"TYPE": "ManoLoss", "LAMBDA_JOINTS_3D": w["mano_j"], "LAMBDA_HAND_VERTS_3D": 0.0, "LAMBDA_SHAPE_REG": w["shape"], "LAMBDA_POSE_REG": w["pose"]},
            {"TYPE": "JointsLoss", "LAMBDA_JOINTS_3D": w["j"], "LAMBDA_CORNERS_3D": w["c"]},
            {"TYPE": "HandOrdLoss", "LAMBDA_JOINTS_LEVEL": w["jo"], "LAMBDA_PART_LEVEL": w["po"]}, {"TYPE": "SceneOrdLoss", "LAMBDA_SCENE_LEVEL": w["so"]}]
    return Criterion({"LAMBDAS": w["LAMBDAS"]}, R.build_criterion_loss_list(cfgc, preset_cfg=preset, LAMBDAS=w["LAMBDAS"]))


def _inputs(B, ncomps, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.06 * torch.randn(B, 21, 3, generator=g), 0.6 * torch.randn(B, 3 + ncomps, generator=g), 0.8 * torch.randn(B, 10, generator=g),
            torch.cat([0.05 * torch.randn(B, 3, generator=g), torch.randn(B, 6, generator=g)], 1))


def _oracle64(joints, pose, shape, transf, batch, w):
    """float64: the regbased assembly (hpregnet.py:112-147) + the pinned losses of learner_oracle + ManoLoss's three terms.  Consumes
    the global RNGs in the reference's order (hand views, joint pairs, part pairs, scene views, scene pairs)."""
    b = {k: v.double() for k, v in batch.items() if k != "image"}
    root = b["root_joint"]
    ja = joints + root[:, None]
    R = lo.ortho6d_to_rotmat(transf[:, 3:9])
    ca = torch.matmul(R, b["corners_can"].permute(0, 2, 1)).permute(0, 2, 1) + (root + transf[:, :3])[:, None]
    preds = {"joints_3d_abs": ja, "corners_3d_abs": ca}
    draws = dict(hand_views=lo.draw_view_vectors(20).double(), joint_sel=lo.draw_pair_subset(len(lo.JOINT_PAIRS)),
                 part_sel=lo.draw_pair_subset(len(lo.PART_PAIRS)), scene_views=lo.draw_view_vectors(40).double(),
                 scene_sel=lo.draw_pair_subset(len(lo.HO_PAIRS)))
    if w is SHIPPED:      # the oracle's own Criterion sum for the shipped inner lambdas (1.0 / 0.2, 1 / 1, 1)
        rest, d, _ = lo.criterion(preds, b, lambdas=tuple(w["LAMBDAS"][1:]), draws=draws)
    else:
        l1, d = lo.joints_loss(preds, b, w["j"], w["c"])
        l2, d2 = lo.hand_ord_loss(preds, b, draws["hand_views"], draws["joint_sel"], draws["part_sel"], w["jo"], w["po"])
        l3, d3 = lo.scene_ord_loss(preds, b, draws["scene_views"], draws["scene_sel"], w["so"])
        d = {**d, **d2, **d3}
        rest = w["LAMBDAS"][1] * l1 + w["LAMBDAS"][2] * l2 + w["LAMBDAS"][3] * l3
    ms, mp = shape.pow(2).mean(), pose[:, 3:].pow(2).mean()
    mj = torch.nn.functional.mse_loss(ja, b["joints_3d"] + root[:, None])
    total = w["LAMBDAS"][0] * (w["shape"] * ms + w["pose"] * mp + w["mano_j"] * mj) + rest
    vec = {0: d["joints_3d_loss"], 1: d["corners_3d_loss"], 2: d["joint_ord_loss"], 3: d["part_ord_loss"], 4: d["scene_ord_loss"], 5: total,
           8: ms, 9: mp, 10: mj}
    return ja, ca, R, total, vec, b


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("ncomps", [15, 45])
@pytest.mark.parametrize("B,seed", [(1, 0), (5, 1), (64, 2)])
def test_reg_pose_loss_kernel_vs_float64(B, seed, ncomps, setting):
    """Tolerances of test_fused_pose_loss_vs_oracle (the same kind of kernel against the same oracle): assembled tensors rtol 1e-5 / atol
    1e-6, loss scalars rtol 2e-5, gradients rtol 2e-4 / atol 2e-5 max|g|, per-sample EPE rtol 1e-4."""
    from artiboost_amd.criterions import FusedRegCriterion
    w = SETTINGS[setting]
    batch = make_batch(B, 224, seed + 10)
    leaves = [t.double().requires_grad_(True) for t in _inputs(B, ncomps, seed)]
    random.seed(seed + 3); torch.manual_seed(seed + 3)
    ja, ca, R, total, vec, b64 = _oracle64(*leaves, batch, w)
    total.backward()
    fused = FusedRegCriterion(_criterion(w), ncomps)
    random.seed(seed + 3); torch.manual_seed(seed + 3)
    fused.draw(torch.device("cuda"))
    joints, pose, shape, transf = [t.detach().float().cuda() for t in leaves]
    tbuf = torch.full((B, 16), 7.0).cuda()          # transf with a row pitch larger than 9
    tbuf[:, :9] = transf
    gbuf = torch.full((B, 16), -3.0).cuda()
    tb = {k: v.cuda() for k, v in batch.items()}
    o = fused(joints, pose, shape, tbuf[:, :9], tb, g_transf=gbuf[:, :9])
    first = {k: v.clone() for k, v in o.items()}
    f32 = lambda t: t.detach().numpy()     # noqa: E731
    np.testing.assert_allclose(o["joints_3d_abs"].cpu().numpy(), f32(ja), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o["corners_3d_abs"].cpu().numpy(), f32(ca), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(o["box_rot_rotmat"].cpu().numpy(), f32(R), rtol=1e-5, atol=1e-6)
    lv = o["losses"].cpu().double().numpy()
    print(f"\n{setting} B={B} ncomps={ncomps}: " + " ".join(f"[{i}] {lv[i]:.9e}/{float(v):.9e}" for i, v in vec.items()))
    for i, v in vec.items():
        np.testing.assert_allclose(lv[i], float(v), rtol=2e-5, err_msg=f"loss slot {i}")
    for name, got, leaf in (("g_joints", o["g_joints"], leaves[0]), ("g_pose", o["g_pose"], leaves[1]), ("g_shape", o["g_shape"], leaves[2]),
                            ("g_transf", gbuf[:, :9], leaves[3])):
        ref = leaf.grad.numpy() if leaf.grad is not None else np.zeros(tuple(leaf.shape))
        print(f"  {name}: max|g| {np.abs(ref).max():.3e} max err {np.abs(got.cpu().double().numpy() - ref).max():.3e}")
        np.testing.assert_allclose(got.cpu().double().numpy(), ref, rtol=2e-4, atol=2e-5 * np.abs(ref).max(), err_msg=name)
    assert torch.equal(gbuf[:, 9:], torch.full((B, 7), -3.0).cuda())          # nothing written beyond the nine values of a row
    epe_j = lo.mean_epe_mm(ja.detach(), b64["joints_3d"], b64["root_joint"])
    epe_c = lo.mean_epe_mm(ca.detach(), b64["corners_3d"], b64["root_joint"])
    np.testing.assert_allclose(o["sample_part"][:, 5].cpu().numpy(), epe_j.numpy(), rtol=1e-4)
    np.testing.assert_allclose(o["sample_part"][:, 6].cpu().numpy(), epe_c.numpy(), rtol=1e-4)
    np.testing.assert_allclose(lv[6], float(epe_j.mean()), rtol=1e-4)
    np.testing.assert_allclose(lv[7], float(epe_c.mean()), rtol=1e-4)
    # forward only (NULL g_joints): the same outputs bit for bit, the gradient buffers untouched
    gkeep = gbuf.clone()
    for k in ("joints_3d_abs", "corners_3d_abs", "box_rot_rotmat", "sample_part", "losses"):
        o[k].fill_(float("nan"))
    o = fused(joints, pose, shape, tbuf[:, :9], tb, backward=False)
    for k in ("joints_3d_abs", "corners_3d_abs", "box_rot_rotmat", "sample_part", "losses"):
        assert torch.equal(o[k], first[k]), k
    assert torch.equal(gbuf, gkeep) and torch.equal(o["g_joints"], first["g_joints"])
    # two calls: identical bits
    for k in o:
        o[k].fill_(float("nan"))
    gbuf.fill_(-3.0)
    o = fused(joints, pose, shape, tbuf[:, :9], tb, g_transf=gbuf[:, :9])
    for k in ("joints_3d_abs", "corners_3d_abs", "box_rot_rotmat", "sample_part", "losses", "g_joints", "g_pose", "g_shape"):
        assert torch.equal(o[k], first[k]), k
    assert torch.equal(gbuf, gkeep)


@pytest.mark.parametrize("setting", ["shipped", "mano_j", "so"])
def test_losses_dict_has_the_registry_routes_entries(setting):
    from artiboost_amd.criterions import FusedRegCriterion
    from artiboost_amd.hpregnet import combine_outputs, mano_outputs, object_outputs
    B, ncomps = 16, 15
    w = SETTINGS[setting]
    crit = _criterion(w)
    batch = {k: v.cuda() for k, v in make_batch(B, 224, 31).items()}
    joints, pose, shape, transf = [t.cuda() for t in _inputs(B, ncomps, 4)]
    mano = {"hand_verts_3d": torch.zeros(B, 778, 3).cuda(), "joints_3d": joints, "mano_shape": shape, "mano_pca_pose": pose,
            "mano_full_pose": torch.zeros(B, 48).cuda()}
    preds = combine_outputs(mano_outputs(mano, batch, "cuda"), object_outputs(transf, batch, "cuda"))
    random.seed(5); torch.manual_seed(5)
    crit.draw(torch.device("cuda"))
    crit.freeze_draws(True)
    try:
        _, ref = crit.compute_losses(preds, batch)
        fused = FusedRegCriterion(crit, ncomps)
        fused(joints, pose, shape, transf, batch)
        got = fused.losses_dict()
    finally:
        crit.freeze_draws(False)
    assert list(sorted(got)) == list(sorted(ref)), (sorted(got), sorted(ref))
    for k, v in ref.items():
        assert (got[k] is None) == (v is None), k
        if v is not None:
            np.testing.assert_allclose(float(got[k]), float(v), rtol=2e-5, err_msg=k)
    assert [k for k in fused.LOSS_KEYS if k is not None] == [k for k in fused.LOSS_KEYS if k is not None and ref[k] is not None]


# ------------------------------------------------------------------------------------------------ the training step
def _step(dtype, size, B, graph, fused=True, lr=3e-4, seed_batch=8, group=None):
    import artiboost_amd.hpregnet  # noqa: F401  (registers HOPRegNet)
    from artiboost_amd import registry as R
    from artiboost_amd.models import Arch
    from artiboost_amd.netutils import build_optimizer
    from artiboost_amd.train import TrainStep
    preset = dict(PRESET, IMAGE_SIZE=[size, size])
    arch = dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE=dtype, INIT_SEED=1, FUSED_STEP=fused)
    model = Arch({"ARCH": arch}, R.build_arch_model_list(arch, preset_cfg=preset))
    crit = _criterion(SHIPPED, preset)
    opt = build_optimizer(model.models_params, OPTIMIZER="adam", LR=lr, WEIGHT_DECAY=0)
    opt.max_norm = 1.0
    batch = {k: v.cuda() for k, v in make_batch(B, size, seed_batch).items()}
    model.train()
    ts = TrainStep(model, crit, opt, batch, use_graph=graph, dist_group=group)
    return model, opt, ts


def _state(ts, opt):
    st = next(iter(opt.state.values()))
    return (ts.hb.store.flat.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), ts.fused.out["losses"].clone(),
            ts.hb.store.stats.clone())


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_graph_replay_equals_the_eager_fused_step_bit_for_bit_and_resumes(dtype, tmp_path):
    runs = {}
    for graph in (False, True):
        model, opt, ts = _step(dtype, 128, 8, graph)
        assert ts.fused is not None and ts.use_graph == graph and not ts.split
        _seed(17)
        seq = []
        for i in range(5):
            ts()
            seq.append(_state(ts, opt))
            if graph and i == 2:           # a checkpoint after step 3: weights + BatchNorm state, optimizer, host RNG streams
                torch.save({"model": ts.hb.state_dict(), "opt": opt.state_dict(),
                            "rng": (random.getstate(), np.random.get_state(), torch.get_rng_state())}, tmp_path / "ck.pth")
        runs[graph] = seq
    for i, (a, b) in enumerate(zip(runs[False], runs[True])):
        for name, x, y in zip(("flat", "exp_avg", "exp_avg_sq", "losses", "bn stats"), a, b):
            assert torch.equal(x, y), (i, name, (x - y).abs().max().item())
    assert torch.isfinite(runs[True][-1][3]).all() and not torch.equal(runs[True][0][0], runs[True][4][0])
    # resume: a fresh model and optimizer, the checkpoint loaded before the first (capturing) step
    ck = torch.load(tmp_path / "ck.pth", weights_only=False)
    model, opt, ts = _step(dtype, 128, 8, True)
    ts.hb.load_state_dict(ck["model"])
    ts.hb.net.pack_weights()
    opt.load_state_dict(ck["opt"])
    random.setstate(ck["rng"][0]); np.random.set_state(ck["rng"][1]); torch.set_rng_state(ck["rng"][2])
    for i in (3, 4):
        ts()
        for name, x, y in zip(("flat", "exp_avg", "exp_avg_sq", "losses", "bn stats"), _state(ts, opt), runs[True][i]):
            assert torch.equal(x, y), (i, name, (x - y).abs().max().item())


def test_fused_route_gradient_vs_the_autograd_route():
    """One f32 step at 128 x 128, B = 8, same weights, batch and draws.  The two routes differ by fp32 rounding inside the criterion; the
    autograd route's index_select backward accumulates with float atomics, so it has a run-to-run spread of its own.
    Bound: max(10 x the measured registry-vs-fused difference, the registry route's own spread), never above 1e-3 (a tenth of what the
    trunk parity tests allow; a wrong head gradient is test_reg_pose_loss_kernel_vs_float64's to catch).
    Measured on MI355X (relative L2 of the whole flat gradient, |g| = 1.225): registry vs registry 2.275e-06, registry vs fused 2.297e-06 --
    the fused route sits inside the autograd route's own run-to-run spread."""
    grads = []
    for fused in (False, False, True):
        model, opt, ts = _step("f32", 128, 8, False, fused=fused)
        assert (ts.fused is not None) == fused
        _seed(23)
        ts._fwd_bwd() if not fused else (ts.crit.draw(ts.dev), ts._fwd_bwd())
        torch.cuda.synchronize()
        grads.append(ts.hb.store.grad.detach().double().clone())
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()      # noqa: E731
    spread, diff = rel(grads[1], grads[0]), rel(grads[2], grads[0])
    print(f"\nregistry vs registry {spread:.3e}, registry vs fused {diff:.3e}, |g| {grads[0].norm().item():.3e}")
    assert grads[0].norm().item() > 0
    bound = min(max(10 * MEASURED_DIFF, MEASURED_SPREAD), 1e-3)
    assert diff <= bound, (diff, bound, spread)


# relative L2 differences of the whole flat gradient measured on MI355X (f32, 128 x 128, B = 8; see the test above and DESIGN.md section 16)
MEASURED_SPREAD = 2.275e-06
MEASURED_DIFF = 2.297e-06       # -> bound 2.297e-05


def test_fused_graph_step_reduces_the_loss_on_a_fixed_batch():
    model, opt, ts = _step("bf16x3", 128, 8, True)
    assert ts.fused is not None and ts.use_graph and ts.model_key == "HOPRegNet"
    vals = []
    for _ in range(40):
        _, losses, _ = ts()
        vals.append(float(losses[5]))
    assert np.isfinite(vals).all(), vals
    assert vals[-1] < 0.5 * vals[0], (vals[0], vals[-1])
    preds = ts.predictions()
    assert len(preds) == 18 and torch.equal(preds["joints_3d_abs"], ts.fused.out["joints_3d_abs"])
    np.testing.assert_allclose(preds["corners_3d_abs"].cpu().numpy(), ts.fused.out["corners_3d_abs"].cpu().numpy(), rtol=1e-5, atol=1e-6)


def test_rccl_single_rank_schedule_regbased():
    """tools/ddp_smoke.py --model regbased under torch.distributed.run with one rank: once with a one-rank nccl group (the unsplit
    schedule: all-reduce between the two graphs), once without a collective.  SUM over one rank x 1.0 is the identity."""
    outs = []
    for i, extra in enumerate(({"AB_DDP_SINGLE_RANK": "1"}, {})):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
        if not extra:
            env.pop("AB_DDP_SINGLE_RANK", None)
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                            "--master-port", str(29561 + i), os.path.join(ROOT, "tools", "ddp_smoke.py"), "--model", "regbased"], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        outs.append([l for l in r.stdout.splitlines() if l.startswith("model=regbased ")][-1])
    assert "backend=nccl world=1" in outs[0] and "comm=True" in outs[0] and "comm=False" in outs[1], outs
    key = lambda l: re.search(r"final_loss=(\S+) weight_sum=(\S+)", l).groups()      # noqa: E731
    assert key(outs[0]) == key(outs[1]), outs


def test_train_script_with_the_fused_regbased_config(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(FUSED_CFG))
    assert cfg["ARCH"]["FUSED_STEP"] is True
    cfg["TRAIN"]["EPOCH"] = 2
    y = tmp_path / "cfg.yaml"
    y.write_text(yaml.dump(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "train", "train_artiboost.py"), "--cfg", str(y), "--gpu_id", "0", "--gpu_render_id", "0",
           "--batch_size", "8", "--exp_id", "t", "--snapshot", "1", "--synth_len", "32", "--size", "64", "--test_freq", "2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 2 and "final_loss" in lines[-1], out.stdout[-2000:]
    assert len([l for l in out.stdout.splitlines() if l.startswith("test ")]) == 1
    exp = [d for d in os.listdir(tmp_path / "exp") if d.startswith("t_")]
    ck = tmp_path / "exp" / exp[0] / "checkpoints" / "checkpoint"
    assert (ck / "HOPRegNet.pth.tar").exists() and (ck / "train_param.pth.tar").exists()
    sd = torch.load(ck / "HOPRegNet.pth.tar", map_location="cpu", weights_only=False)
    import artiboost_amd.hpregnet as H
    from artiboost_amd import registry as R
    cpu = R.build_arch_model_list({k: v for k, v in cfg["ARCH"].items() if k != "FUSED_STEP"}, preset_cfg=cfg["DATA_PRESET"])[0]
    assert isinstance(cpu, H.HOPRegNet)
    cpu.load_state_dict(H.HOPRegNet.clean_reference_state_dict(sd), strict=True)
    out = subprocess.run(cmd + ["--resume", str(tmp_path / "exp" / exp[0])], capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]


def test_deferred_epoch_metrics_equal_per_step_feeding():
    from artiboost_amd import registry as R
    from artiboost_amd.metrics import Evaluator
    from artiboost_amd.train import DeferredEpochMetrics
    ev_cfg = [{"TYPE": "LossesMetric", "VIS_LOSS_KEYS": []}, {"TYPE": "Mean3DEPE", "VAL_KEYS": ["corners_3d_abs", "joints_3d_abs"], "MILLIMETERS": True},
              {"TYPE": "ValMetricMean3DEPE2", "VAL_KEYS": ["corners_3d_abs", "joints_3d_abs"], "MILLIMETERS": True}]
    mk = lambda: Evaluator({}, R.build_evaluator_metric_list(copy.deepcopy(ev_cfg), preset_cfg=PRESET), max_lag=0)      # noqa: E731
    deferred, direct = mk(), mk()
    model, opt, ts = _step("bf16x3", 128, 8, True)
    B = 8
    rec = DeferredEpochMetrics(ts, 4, deferred)
    assert rec.losses.shape[1] == ts.fused.LOSS_WIDTH and not rec.direct
    g = torch.Generator().manual_seed(1)
    for s in range(4):
        ts.static["obj_id"] = torch.randint(0, 3, (B,), generator=g).cuda()
        ts.static["persp_id"] = torch.randint(0, 2, (B,), generator=g).cuda()
        ts.static["grasp_id"] = torch.randint(0, 2, (B,), generator=g).cuda()
        ts.static["is_synth"] = (torch.rand(B, generator=g) > 0.3).cuda()
        ts()
        rec.collect()
        direct.feed_all(ts.predictions(), ts.static, ts.fused.losses_dict())
    rec.flush(deferred)
    for a, b in zip(deferred.metrics_list, direct.metrics_list):
        assert type(a) is type(b)
        if hasattr(a, "meters"):          # LossesMetric
            assert set(a.meters) == set(b.meters)
            for k in b.meters:
                np.testing.assert_allclose(a.meters[k].avg, b.meters[k].avg, rtol=1e-6, err_msg=k)
        elif hasattr(a, "storage"):       # ValMetricMean3DEPE2: last write per CCV triplet
            for k in b.storage:
                assert set(a.storage[k]) == set(b.storage[k])
                for t in b.storage[k]:
                    np.testing.assert_allclose(float(a.storage[k][t]), float(b.storage[k][t]), rtol=1e-5)
        else:                             # Mean3DEPE
            for k in b.avg_meters:
                np.testing.assert_allclose(a.avg_meters[k].avg, b.avg_meters[k].avg, rtol=1e-5, err_msg=k)
