"""HoNet's fused mesh criterion and graph-replayed training step (ARCH.FUSED_MESH_STEP): ab_mesh_queries against a float64 restatement of
synth.add_mesh_queries; ab_honet_loss / FusedMeshCriterion against criterions.ManoLoss + ObjLoss on double tensors, term by term; its loss
dict against the registry losses; graph replay against the eager fused route bit for bit, with the in-graph mesh queries and a resumed
checkpoint; the fused route's gradient against the autograd route's; training on a fixed batch; DeferredEpochMetrics against per-step
feeding; the one-rank RCCL schedule; the training script with the shipped config."""
import copy
import os
import random
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import learner_oracle as lo
from gen_batch import make_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_CFG = os.path.join(ROOT, "config", "ho3dv2_honet_mi355x_fused.yaml")
BOUND_3D = 2e-6          # metres: the bound test_gpu_honet.py holds the recovery forward to (same magnitudes, same three-term dot products)


# ------------------------------------------------------------------------------------------------ ab_mesh_queries
def _mq_case(B, n, pitch, seed):
    """A vertex table of four objects (object 1 has fewer than n vertices whenever n > 1, so its rows repeat), B samples around 0.5 m
    whose ids include the short object and, from B = 5, one id above and one below the table."""
    from artiboost_amd.render import SAMPLE_DTYPE
    from artiboost_amd.synth import mesh_vertex_table
    rng = np.random.default_rng(seed)
    counts = [3 * n + 7, max(1, n // 2), n, 2 * n + 3]
    off = np.concatenate([[0], np.cumsum(counts)])
    assets = SimpleNamespace(n_obj=4, obj_verts=(0.08 * rng.standard_normal((off[-1], 3))).astype(np.float32), obj_vert_off=off)
    table = mesh_vertex_table(assets, n)
    if n > 1:
        assert np.array_equal(table[1, 0], table[1, counts[1]])        # the short object's vertices repeat
    rot = lambda: np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(B)])      # noqa: E731
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, :3, :3] = rot()
    T[:, :3, 3] = [0.0, 0.0, 0.5] + 0.05 * rng.standard_normal((B, 3))
    pose = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    pose[:, :3, :3] = rot()
    pose[:, :3, 3] = rng.standard_normal((B, 3))                       # (the translation of the record is not read)
    rec = np.zeros(B, SAMPLE_DTYPE)
    rec["obj_pose"] = pose.reshape(B, 16)
    raw = np.full((B, pitch), 0xA5, np.uint8)
    raw[:, :96] = rec.view(np.uint8).reshape(B, 96)
    ids = np.array([1, 0, 7, -2, 3][:B], np.int64)
    root = ([0.0, 0.0, 0.5] + 0.05 * rng.standard_normal((B, 3))).astype(np.float32)
    hv = ([0.0, 0.0, 0.5] + 0.05 * rng.standard_normal((B, 778, 3))).astype(np.float32)
    return table, ids, T, root, hv, raw, pose, SAMPLE_DTYPE.fields["obj_pose"][1]


@pytest.mark.parametrize("n", [1, 157, 300])
@pytest.mark.parametrize("B,pitch", [(1, 96), (5, 112)])
def test_mesh_queries_kernel_vs_float64(B, pitch, n):
    from artiboost_amd import kernels as K
    table, ids, T, root, hv, raw, pose, off = _mq_case(B, n, pitch, seed=10 * B + n)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    out = tuple(torch.full(s, float("nan"), device="cuda") for s in ((B, n, 3), (B, n, 3), (B, 778, 3)))
    got = K.mesh_queries(t(table), t(ids), t(T), t(root), t(hv), t(raw), off, out=out)
    assert all(a is b for a, b in zip(got, out))
    # float64 restatement of synth.add_mesh_queries, the id clamped into the table
    can = table[np.clip(ids, 0, 3)]
    T64, R = T.astype(np.float64), T[:, :3, :3].astype(np.float64)
    v3d = np.einsum("bij,bnj->bni", R, can.astype(np.float64)) + T64[:, None, :3, 3] - root[:, None].astype(np.float64)
    rm = R @ pose[:, :3, :3].astype(np.float64).transpose(0, 2, 1)
    h3d = np.einsum("bij,bnj->bni", rm, hv.astype(np.float64)) - root[:, None].astype(np.float64)
    assert torch.equal(got[0].cpu(), torch.from_numpy(can))                                   # bit copies of the table rows
    e_obj = np.abs(got[1].cpu().double().numpy() - v3d).max()
    e_hand = np.abs(got[2].cpu().double().numpy() - h3d).max()
    print(f"\nB={B} n={n}: max err obj_verts_3d {e_obj:.3e} hand_verts_3d {e_hand:.3e}")
    assert e_obj <= BOUND_3D and e_hand <= BOUND_3D, (e_obj, e_hand)
    # the allocating form: the same bits
    again = K.mesh_queries(t(table), t(ids), t(T), t(root), t(hv), t(raw), off)
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_mesh_queries_refuses_a_misaligned_record_layout():
    from artiboost_amd import kernels as K
    table, ids, T, root, hv, raw, pose, off = _mq_case(2, 4, 96, seed=3)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    with pytest.raises(RuntimeError):
        K.mesh_queries(t(table), t(ids), t(T), t(root), t(hv), t(raw), off + 2)          # not a multiple of 4
    with pytest.raises(RuntimeError):
        K.mesh_queries(t(table), t(ids), t(T), t(root), t(hv), t(raw), 64)               # the 4x4 would reach past its record
    with pytest.raises(ValueError):
        K.mesh_queries(t(table), t(ids.astype(np.int32)), t(T), t(root), t(hv), t(raw), off)


# ------------------------------------------------------------------------------------------------ ab_honet_loss
# the shipped loss set (config/ho3dv2_honet_mi355x.yaml), and each of the five terms alone (its lambda 1, its loss's LAMBDA 1, the rest 0)
SHIPPED = dict(shape=5.0e-7, pose=5.0e-6, j=1.0, v=1.0, o=1.0, LAMBDAS=[1.0, 1.0])
ZERO = dict(shape=0.0, pose=0.0, j=0.0, v=0.0, o=0.0)
SETTINGS = {"shipped": SHIPPED, **{t: dict(ZERO, **{t: 1.0}, LAMBDAS=[0.0, 1.0] if t == "o" else [1.0, 0.0]) for t in ZERO}}
G_NAMES = ("g_joints_3d_abs", "g_hand_verts_3d_abs", "g_obj_verts_3d_abs", "g_mano_pca_pose", "g_mano_shape")


def _criterion(w, with_obj=True):
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    cfgc = [{"TYPE": "ManoLoss", "LAMBDA_JOINTS_3D": w["j"], "LAMBDA_HAND_VERTS_3D": w["v"], "LAMBDA_SHAPE_REG": w["shape"], "LAMBDA_POSE_REG": w["pose"]}]
    if with_obj:
        cfgc.append({"TYPE": "ObjLoss", "LAMBDA_OBJ_VERTS_3D": w["o"]})
    lam = w["LAMBDAS"][:len(cfgc)]
    return Criterion({"LAMBDAS": lam}, R.build_criterion_loss_list(cfgc, preset_cfg={}, LAMBDAS=lam))


def _chunk():
    from artiboost_amd import _lib
    nc = _lib.cdll().ab_honet_loss_chunks
    return next(n for n in range(1, 1 << 16) if nc(n + 1) == 2)


def _loss_case(B, N, ncomps, seed):
    """Seeded float32 CPU tensors: targets root-relative around a root at ~0.5 m, predictions 6 cm (rms) off them."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    root = torch.tensor([0.0, 0.0, 0.5]) + 0.05 * r(B, 3)
    targs = {"root_joint": root, "joints_3d": 0.06 * r(B, 21, 3), "hand_verts_3d": 0.06 * r(B, 778, 3), "obj_verts_3d": 0.08 * r(B, N, 3),
             "corners_3d": 0.08 * r(B, 8, 3)}
    preds = {k + "_abs": targs[k] + root[:, None] + 0.06 * r(*targs[k].shape) for k in ("joints_3d", "hand_verts_3d", "obj_verts_3d", "corners_3d")}
    preds["mano_pca_pose"], preds["mano_shape"] = 0.6 * r(B, 3 + ncomps), 0.8 * r(B, 10)
    return preds, targs


LEAVES = ("joints_3d_abs", "hand_verts_3d_abs", "obj_verts_3d_abs", "mano_pca_pose", "mano_shape")


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("ncomps", [15, 45])
@pytest.mark.parametrize("B,seed", [(1, 0), (5, 1), (64, 2)])
def test_honet_loss_kernel_vs_float64(B, seed, ncomps, setting):
    """Tolerances of test_reg_pose_loss_kernel_vs_float64 (the same kind of kernel against the same kind of oracle): loss scalars rtol 2e-5,
    gradients rtol 2e-4 / atol 2e-5 max|g|, per-sample EPE rtol 1e-4.  N = 1 and one below, at and one above the kernel's vertex chunk."""
    from artiboost_amd.criterions import FusedMeshCriterion
    w = SETTINGS[setting]
    crit = _criterion(w)
    chunk = _chunk()
    for N in (1, chunk - 1, chunk, chunk + 1):
        preds, targs = _loss_case(B, N, ncomps, seed + N)
        # float64 oracle: criterions.ManoLoss / ObjLoss themselves on double tensors, through Criterion's own sum
        p64 = {k: v.double().requires_grad_(k in LEAVES) for k, v in preds.items()}
        t64 = {k: v.double() for k, v in targs.items()}
        total, ref = crit.compute_losses(p64, t64)
        total.backward()
        epe_j = lo.mean_epe_mm(p64["joints_3d_abs"].detach(), t64["joints_3d"], t64["root_joint"])
        epe_c = lo.mean_epe_mm(p64["corners_3d_abs"].detach(), t64["corners_3d"], t64["root_joint"])
        pd = {k: v.cuda() for k, v in preds.items()}
        for corners in (True, False):
            td = {k: v.cuda() for k, v in targs.items() if corners or k != "corners_3d"}
            fused = FusedMeshCriterion(crit, ncomps, td)
            args = (pd["joints_3d_abs"], pd["hand_verts_3d_abs"], pd["obj_verts_3d_abs"], pd["corners_3d_abs"] if corners else None,
                    pd["mano_pca_pose"], pd["mano_shape"], td)
            o = fused(*args)
            first = {k: v.clone() for k, v in o.items() if v is not None}
            lv = o["losses"].cpu().double().numpy()
            slots = dict(mano_shape=0, mano_pca_pose=1, joints_3d_loss=2, hand_verts_3d_loss=3, obj_verts_3d_loss=4, final_loss=5)
            print(f"\n{setting} B={B} ncomps={ncomps} N={N} corners={corners}: " +
                  " ".join(f"{k} {lv[s]:.9e}/{('None' if ref[k] is None else format(float(ref[k]), '.9e'))}" for k, s in slots.items()))
            for k, s in slots.items():
                assert (fused.key_slots[k] is None) == (ref[k] is None), k
                if ref[k] is not None:
                    np.testing.assert_allclose(lv[s], float(ref[k]), rtol=2e-5, err_msg=k)
            for name, leaf in zip(G_NAMES, LEAVES):
                gref = p64[leaf].grad.numpy() if p64[leaf].grad is not None else np.zeros(tuple(p64[leaf].shape))
                got = o[name].cpu().double().numpy()
                print(f"  {name}: max|g| {np.abs(gref).max():.3e} max err {np.abs(got - gref).max():.3e}")
                np.testing.assert_allclose(got, gref, rtol=2e-4, atol=2e-5 * np.abs(gref).max(), err_msg=name)
            assert torch.equal(o["g_mano_pca_pose"][:, :3], torch.zeros(B, 3, device="cuda"))      # the root rotation is not regularised
            np.testing.assert_allclose(o["sample_part"][:, 5].cpu().numpy(), epe_j.numpy(), rtol=1e-4)
            np.testing.assert_allclose(lv[6], float(epe_j.mean()), rtol=1e-4)
            if corners:
                np.testing.assert_allclose(o["sample_part"][:, 6].cpu().numpy(), epe_c.numpy(), rtol=1e-4)
                np.testing.assert_allclose(lv[7], float(epe_c.mean()), rtol=1e-4)
            else:
                assert float(o["sample_part"][:, 6].abs().max()) == 0.0 and lv[7] == 0.0
            # forward only (NULL gradient pointers): the same loss bits, the gradient buffers untouched
            for k in ("sample_part", "losses"):
                o[k].fill_(float("nan"))
            for k in G_NAMES:
                o[k].fill_(-3.0)
            o = fused(*args, backward=False)
            assert torch.equal(o["losses"], first["losses"]) and torch.equal(o["sample_part"], first["sample_part"])
            assert all(bool((o[k] == -3.0).all()) for k in G_NAMES)
            # a repeated call: identical bits everywhere
            for k in ("sample_part", "losses"):
                o[k].fill_(float("nan"))
            o = fused(*args)
            for k in ("sample_part", "losses") + G_NAMES:
                assert torch.equal(o[k], first[k]), k


def test_honet_loss_with_mano_loss_alone_reads_no_object_tensor():
    from artiboost_amd.criterions import FusedMeshCriterion
    preds, targs = _loss_case(5, 7, 15, 9)
    crit = _criterion(SHIPPED, with_obj=False)
    p64 = {k: v.double() for k, v in preds.items()}
    total, ref = crit.compute_losses(p64, {k: v.double() for k, v in targs.items()})
    pd, td = {k: v.cuda() for k, v in preds.items()}, {k: v.cuda() for k, v in targs.items()}
    fused = FusedMeshCriterion(crit, 15, td)
    o = fused(pd["joints_3d_abs"], pd["hand_verts_3d_abs"], pd["obj_verts_3d_abs"], pd["corners_3d_abs"], pd["mano_pca_pose"], pd["mano_shape"], td)
    assert o["g_obj_verts_3d_abs"] is None and "obj_verts_3d_loss" not in fused.key_slots
    np.testing.assert_allclose(float(o["losses"][5]), float(total), rtol=2e-5)
    got = fused.losses_dict()
    assert list(got) == list(ref)


# ------------------------------------------------------------------------------------------------ dict parity
@pytest.mark.parametrize("variant", ["shipped", "verts_off", "no_obj_target", "no_joint_target"])
def test_losses_dict_has_the_registry_routes_entries(variant):
    from artiboost_amd.criterions import FusedMeshCriterion
    w = dict(SHIPPED, v=0.0, shape=0.0) if variant == "verts_off" else SHIPPED
    crit = _criterion(w)
    preds, targs = _loss_case(16, 300, 15, 4)
    drop = {"no_obj_target": "obj_verts_3d", "no_joint_target": "joints_3d"}.get(variant)
    pd = {k: v.cuda() for k, v in preds.items()}
    td = {k: v.cuda() for k, v in targs.items() if k != drop}
    _, ref = crit.compute_losses(pd, td)
    fused = FusedMeshCriterion(crit, 15, td)
    fused(pd["joints_3d_abs"], pd["hand_verts_3d_abs"], pd["obj_verts_3d_abs"], pd["corners_3d_abs"], pd["mano_pca_pose"], pd["mano_shape"], td)
    got = fused.losses_dict()
    assert list(got) == list(ref), (list(got), list(ref))
    assert any(v is None for v in ref.values()) == (variant != "shipped")
    for k, v in ref.items():
        assert (got[k] is None) == (v is None), k
        if v is not None:
            np.testing.assert_allclose(float(got[k]), float(v), rtol=2e-5, err_msg=k)
    assert [k for k in fused.LOSS_KEYS if k is not None] == [k for k in ref if ref[k] is not None]


# ------------------------------------------------------------------------------------------------ the training step
ARCH = {"TYPE": "HoNet", "PRETRAINED": "", "PREVIOUS": [], "OBJ_TRANS_FACTOR": 100, "OBJ_SCALE_FACTOR": 0.0001,
        "BACKBONE": {"TYPE": "ResNet18", "PRETRAINED": False, "FREEZE_BATCHNORM": False},
        "HEAD": {"TYPE": "ManoBranch", "MANO_ASSETS_ROOT": "assets/mano_v1_2", "INPUT_DIM": 512, "NCOMPS": 15, "USE_PCA": True, "USE_SHAPE": True}}
PRESET = {"IMAGE_SIZE": [128, 128], "HEATMAP_SIZE": [16, 16], "CENTER_IDX": 0}
N_MESH = 157
_ASSETS = []


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def _batch(B, seed, N=N_MESH):
    b = make_batch(B, 128, seed)
    g = torch.Generator().manual_seed(seed + 1)
    b["obj_verts_can"] = 0.06 * torch.randn(B, N, 3, generator=g)
    b["obj_verts_3d"] = b["obj_verts_can"] + 0.05 * torch.randn(B, 1, 3, generator=g)
    b["hand_verts_3d"] = 0.05 * torch.randn(B, 778, 3, generator=g)
    return b


def _model(dtype, fused):
    import artiboost_amd.honet  # noqa: F401  (registers HoNet)
    from artiboost_amd import registry as R
    from artiboost_amd.models import Arch
    from artiboost_amd.netutils import build_optimizer
    arch = dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE=dtype, INIT_SEED=1, **({"FUSED_MESH_STEP": True} if fused else {}))
    model = Arch({"ARCH": arch}, R.build_arch_model_list(arch, preset_cfg=PRESET))
    opt = build_optimizer(model.models_params, OPTIMIZER="adam", LR=3e-4, WEIGHT_DECAY=0)
    opt.max_norm = 1.0
    model.train()
    return model, opt


def _step(dtype, graph, fused=True, B=8, seed_batch=8, group=None):
    """A TrainStep on a fixed batch that carries the mesh queries itself (no renderer)."""
    from artiboost_amd.train import TrainStep
    model, opt = _model(dtype, fused)
    batch = {k: v.cuda() for k, v in _batch(B, seed_batch).items()}
    ts = TrainStep(model, _criterion(SHIPPED), opt, batch, use_graph=graph, dist_group=group)
    return model, opt, ts


def _loader_step(dtype, graph, B=8):
    """A TrainStep fed by a synthetic loader with MANAGER.MESH_QUERIES: render + mesh queries + learn inside the step."""
    import yaml
    from artiboost_amd.assets import SceneAssets
    from artiboost_amd.synth import ArtiBoostLoader
    from artiboost_amd.train import TrainStep
    if not _ASSETS:
        _ASSETS.append(SceneAssets("HO3D", seed=1))
    cfg = yaml.safe_load(open(FUSED_CFG))
    _seed(5)
    model, opt = _model(dtype, True)
    loader = ArtiBoostLoader.from_assets(_ASSETS[0], dict(cfg["MANAGER"], MESH_QUERIES=N_MESH, EPOCH=1), PRESET, B, B * 5, device="cuda",
                                         compute_dtype=model.model_list[0].net.dtype, random_seed=1)
    loader.prepare()
    static = loader.new_static_batch()
    loader.load_batch(static, 0)
    ts = TrainStep(model, _criterion(SHIPPED), opt, static, use_graph=graph, renderer=loader)
    return loader, opt, ts


def _state(ts, opt):
    st = next(iter(opt.state.values()))
    return (ts.hb.store.flat.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), ts.fused.out["losses"].clone(),
            ts.hb.store.stats.clone())


NAMES = ("flat", "exp_avg", "exp_avg_sq", "losses", "bn stats")


@pytest.mark.parametrize("dtype", ["f32", "bf16x3"])
def test_graph_replay_equals_the_eager_fused_step_bit_for_bit_and_resumes(dtype, tmp_path):
    runs = {}
    for graph in (False, True):
        loader, opt, ts = _loader_step(dtype, graph)
        assert ts.fused is not None and ts.mesh and ts.mesh_queries and ts.use_graph == graph and not ts.split
        # the recovery stage reads the static tensors themselves
        geo = ts.hb._geo_of(ts.static)
        assert geo[0] is ts.static["cam_intr"] and geo[1] is ts.static["obj_verts_can"] and geo[2] is ts.static["corners_can"]
        _seed(17)
        seq = []
        for i in range(5):
            ts.stage(loader, i)
            ts()
            seq.append(_state(ts, opt))
            # the in-step mesh queries against the eager torch route on the same staged batch
            items = {k: v for k, v in ts.static.items() if not k.startswith("_") and k not in loader.MESH_QUERY_KEYS}
            loader.add_mesh_queries(items, ts.static)
            assert torch.equal(ts.static["obj_verts_can"], items["obj_verts_can"]) and ts.static["obj_verts_can"].shape == (8, N_MESH, 3)
            for k in ("obj_verts_3d", "hand_verts_3d"):
                err = (ts.static[k] - items[k]).abs().max().item()
                assert err <= BOUND_3D, (i, k, err)
            if graph and i == 2:           # a checkpoint after step 3: weights + BatchNorm state, optimizer, host RNG streams
                torch.save({"model": ts.hb.state_dict(), "opt": opt.state_dict(),
                            "rng": (random.getstate(), np.random.get_state(), torch.get_rng_state())}, tmp_path / "ck.pth")
        runs[graph] = seq
    for i, (a, b) in enumerate(zip(runs[False], runs[True])):
        for name, x, y in zip(NAMES, a, b):
            assert torch.equal(x, y), (i, name, (x - y).abs().max().item())
    assert torch.isfinite(runs[True][-1][3]).all() and not torch.equal(runs[True][0][0], runs[True][4][0])
    assert not torch.equal(runs[True][0][3], runs[True][1][3])              # (the batches differ from step to step)
    # resume: a fresh model and optimizer, the checkpoint loaded before the first (capturing) step
    ck = torch.load(tmp_path / "ck.pth", weights_only=False)
    loader, opt, ts = _loader_step(dtype, True)
    ts.hb.load_state_dict(ck["model"])
    ts.hb.net.pack_weights()
    opt.load_state_dict(ck["opt"])
    random.setstate(ck["rng"][0]); np.random.set_state(ck["rng"][1]); torch.set_rng_state(ck["rng"][2])
    for i in (3, 4):
        ts.stage(loader, i)
        ts()
        for name, x, y in zip(NAMES, _state(ts, opt), runs[True][i]):
            assert torch.equal(x, y), (i, name, (x - y).abs().max().item())


FLOOR = 2.3e-5           # the figure test_gpu_reg_criterion.py holds the regbased twin to on the same trunk


def test_fused_route_gradient_vs_the_autograd_route():
    """One f32 step at 128 x 128, B = 8, same weights and batch: the whole flat gradient, relative L2.  The two routes differ by fp32
    rounding inside the criterion and by the order in which the recovery stage's gradients are summed.  Bound: 10 x the autograd route's
    own run-to-run spread, measured here, and not below FLOOR (the floor decides if HoNet's autograd route is bit-reproducible).
    The test prints both figures; they have not been recorded from an MI355X run yet."""
    grads = []
    for fused in (False, False, True):
        model, opt, ts = _step("f32", False, fused=fused)
        assert (ts.fused is not None) == fused and not ts.use_graph
        _seed(23)
        ts._fwd_bwd()
        torch.cuda.synchronize()
        grads.append(ts.hb.store.grad.detach().double().clone())
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()      # noqa: E731
    spread, diff = rel(grads[1], grads[0]), rel(grads[2], grads[0])
    print(f"\nregistry vs registry {spread:.3e}, registry vs fused {diff:.3e}, |g| {grads[0].norm().item():.3e}")
    assert grads[0].norm().item() > 0
    bound = max(10 * spread, FLOOR)
    assert diff <= bound, (diff, bound, spread)


def test_fused_graph_step_reduces_the_loss_on_a_fixed_batch():
    model, opt, ts = _step("bf16x3", True)
    assert ts.fused is not None and ts.use_graph and ts.model_key == "HoNet" and not ts.mesh_queries
    vals = []
    for _ in range(8):
        out, losses, _ = ts()
        vals.append(float(losses[5]))
    assert np.isfinite(vals).all(), vals
    assert vals[-1] < vals[0], vals
    # predictions(): the model's own dict, key for key, over the step's outputs
    preds = ts.predictions()
    with torch.no_grad():
        ref = ts.hb(ts.static)
    assert list(preds) == list(ref) and all((preds[k] is None) == (ref[k] is None) for k in ref)
    assert preds["joints_3d_abs"] is out[7 + 1] and preds["mano_pca_pose"] is out[0] and preds["boxroot_3d_abs"] is preds["obj_center"]
    # the criterion's EPE column is the evaluator's definition on those predictions
    epe = lo.mean_epe_mm(preds["joints_3d_abs"].cpu().double(), ts.static["joints_3d"].cpu().double(), ts.static["root_joint"].cpu().double())
    np.testing.assert_allclose(ts.fused.out["sample_part"][:, 5].cpu().numpy(), epe.numpy(), rtol=1e-4)


def test_deferred_epoch_metrics_equal_per_step_feeding():
    from artiboost_amd import registry as R
    from artiboost_amd.metrics import Evaluator
    from artiboost_amd.train import DeferredEpochMetrics
    ev_cfg = [{"TYPE": "LossesMetric", "VIS_LOSS_KEYS": []}, {"TYPE": "Mean3DEPE", "VAL_KEYS": ["corners_3d_abs", "joints_3d_abs"], "MILLIMETERS": True},
              {"TYPE": "ValMetricMean3DEPE2", "VAL_KEYS": ["corners_3d_abs", "joints_3d_abs"], "MILLIMETERS": True}]
    mk = lambda: Evaluator({}, R.build_evaluator_metric_list(copy.deepcopy(ev_cfg), preset_cfg=PRESET), max_lag=0)      # noqa: E731
    deferred, direct = mk(), mk()
    model, opt, ts = _step("bf16x3", True)
    B = 8
    rec = DeferredEpochMetrics(ts, 4, deferred)
    assert rec.losses.shape[1] == ts.fused.LOSS_WIDTH == 8 and not rec.direct
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
            assert set(a.meters) == set(b.meters) and "obj_verts_3d_loss" in a.meters and "hand_verts_3d_loss" in a.meters
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


def test_rccl_single_rank_schedule_honet():
    """tools/ddp_smoke.py --model honet under torch.distributed.run with one rank: once with a one-rank nccl group (the unsplit schedule:
    all-reduce between the two graphs), once without a collective.  SUM over one rank x 1.0 is the identity."""
    outs = []
    for i, extra in enumerate(({"AB_DDP_SINGLE_RANK": "1"}, {})):
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra)
        if not extra:
            env.pop("AB_DDP_SINGLE_RANK", None)
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                            "--master-port", str(29571 + i), os.path.join(ROOT, "tools", "ddp_smoke.py"), "--model", "honet"], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
        outs.append([l for l in r.stdout.splitlines() if l.startswith("model=honet ")][-1])
    assert "backend=nccl world=1" in outs[0] and "comm=True" in outs[0] and "comm=False" in outs[1], outs
    key = lambda l: re.search(r"final_loss=(\S+) weight_sum=(\S+)", l).groups()      # noqa: E731
    assert key(outs[0]) == key(outs[1]), outs


def test_train_script_with_the_fused_honet_config(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(FUSED_CFG))
    assert cfg["ARCH"]["FUSED_MESH_STEP"] is True and cfg["MANAGER"]["MESH_QUERIES"] > 0
    cfg["TRAIN"]["EPOCH"] = 1
    y = tmp_path / "cfg.yaml"
    y.write_text(yaml.dump(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "train", "train_artiboost.py"), "--cfg", str(y), "--gpu_id", "0", "--gpu_render_id", "0",
           "--batch_size", "8", "--exp_id", "t", "--snapshot", "1", "--synth_len", "16", "--size", "64"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 1 and "final_loss" in lines[-1], out.stdout[-2000:]
    exp = [d for d in os.listdir(tmp_path / "exp") if d.startswith("t_")]
    ck = tmp_path / "exp" / exp[0] / "checkpoints" / "checkpoint"
    sd = torch.load(ck / "HoNet.pth.tar", map_location="cpu", weights_only=False)
    assert "obj_transhead.final_layer.weight" in sd and all(torch.isfinite(v).all() for v in sd.values() if v.dtype.is_floating_point)
