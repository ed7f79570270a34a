"""Mesh queries of REAL frames on the device: ab_real_mesh_queries against float64; RealBatcher(mesh_queries=n) over the
miniature HO3D tree against the float64 chain through pose_oracle.mano_lbs, every other key unchanged; MixedLoader's two halves and the
threaded prefetcher; HoNet's forward on a real-only batch and its fused, graph-replayed step over mixed batches; the training script with
the fused HoNet config on a tree with real frames."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import ho3d_fake_tree as T
import pose_oracle as po

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED_CFG = os.path.join(ROOT, "config", "ho3dv2_honet_mi355x_fused.yaml")
BOUND_3D = 2e-6          # metres: the bound ab_mesh_queries is held to at the same magnitudes (tests/test_gpu_honet_criterion.py)
BOUND_MANO = 2e-6        # metres: test_mano_lbs_vs_oracle's bound on ab_mano_lbs
N_MESH = 157
PRESET = {"USE_CACHE": True, "FILTER_NO_CONTACT": False, "FILTER_THRESH": 0.0, "BBOX_EXPAND_RATIO": 1.2, "FULL_IMAGE": False,
          "IMAGE_SIZE": [128, 128], "HEATMAP_SIZE": [16, 16], "CENTER_IDX": 0, "CROP_MODEL": "root_obj"}
E = np.diag([1.0, -1.0, -1.0])
_ASSETS = []


def _seed(s):
    random.seed(s); np.random.seed(s); torch.manual_seed(s)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ ab_real_mesh_queries
def _maps(rng, B):
    """[B,3,4] maps of the shape real_mesh_maps composes: a 0.6 rad in-plane rotation times a flip (odd samples) times a rotation, and a
    translation that keeps the placed points within 1 m."""
    c, s = np.cos(0.6), np.sin(0.6)
    rm = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    m = np.zeros((B, 3, 4))
    for b in range(B):
        F = np.diag([-1.0, 1.0, 1.0]) if b % 2 else np.eye(3)
        m[b, :, :3] = rm @ F @ np.linalg.qr(rng.standard_normal((3, 3)))[0]
        m[b, :, 3] = rng.uniform(-0.4, 0.4, 3)
    return m.astype(np.float32)


@pytest.mark.parametrize("n", [1, 157, 300])
@pytest.mark.parametrize("B", [1, 5])
def test_real_mesh_queries_kernel_vs_float64(B, n):
    from artiboost_amd import kernels as K
    rng = np.random.default_rng(100 * B + n)
    table = (0.08 * rng.standard_normal((3, n, 3))).astype(np.float32)
    row = np.array([-1, 3, 1, 0, 2][:B], np.int64)                       # -1 and n_rows: clamped into the table
    obj_map, hand_map = _maps(rng, B), _maps(rng, B)
    mv = (0.08 * rng.standard_normal((B, 778, 3))).astype(np.float32)
    out = tuple(torch.full(s, float("nan"), device="cuda") for s in ((B, n, 3), (B, n, 3), (B, 778, 3)))
    got = K.real_mesh_queries(t(table), t(row), t(obj_map), t(hand_map), t(mv), out=out)
    assert all(a is b for a, b in zip(got, out))
    can = table[np.clip(row, 0, 2)]
    ap = lambda m, p: np.einsum("bij,bnj->bni", m[:, :, :3].astype(np.float64), p.astype(np.float64)) + m[:, None, :, 3].astype(np.float64)      # noqa: E731
    np.testing.assert_array_equal(got[0].cpu().numpy(), can)              # bit copies of the table rows
    e_obj = np.abs(got[1].cpu().double().numpy() - ap(obj_map, can)).max()
    e_hand = np.abs(got[2].cpu().double().numpy() - ap(hand_map, mv)).max()
    print(f"\nB={B} n={n}: max err obj_verts_3d {e_obj:.3e} hand_verts_3d {e_hand:.3e}")
    assert np.abs(ap(obj_map, can)).max() < 1.0 and np.abs(ap(hand_map, mv)).max() < 1.0
    assert e_obj <= BOUND_3D and e_hand <= BOUND_3D, (e_obj, e_hand)
    again = K.real_mesh_queries(t(table), t(row), t(obj_map), t(hand_map), t(mv))      # the allocating form, a second call: the same bits
    assert all(torch.equal(a, b) for a, b in zip(again, got))


def test_real_mesh_queries_with_an_empty_batch_and_bad_arguments():
    from artiboost_amd import kernels as K
    z = lambda *s: torch.zeros(s, device="cuda")      # noqa: E731
    table = z(3, 7, 3)
    got = K.real_mesh_queries(table, torch.zeros(0, dtype=torch.int64, device="cuda"), z(0, 3, 4), z(0, 3, 4), z(0, 778, 3))
    torch.cuda.synchronize()
    assert [tuple(g.shape) for g in got] == [(0, 7, 3), (0, 7, 3), (0, 778, 3)]
    with pytest.raises(ValueError):
        K.real_mesh_queries(table, torch.zeros(2, dtype=torch.int32, device="cuda"), z(2, 3, 4), z(2, 3, 4), z(2, 778, 3))
    with pytest.raises(ValueError):
        K.real_mesh_queries(table, torch.zeros(2, dtype=torch.int64, device="cuda"), z(2, 3, 3), z(2, 3, 4), z(2, 778, 3))


# ------------------------------------------------------------------------------------------------ RealBatcher
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("ho3d")
    T.build(str(root), seed=7)
    return str(root)


@pytest.fixture(scope="module")
def hand():
    from artiboost_amd.assets import make_hand_model
    return make_hand_model(1)


def _ds(tree, split="train"):
    from artiboost_amd import datasets as D
    return D.HO3D(DATA_ROOT=tree, DATA_SPLIT=split, SPLIT_MODE="paper", AUG=split == "train", AUG_PARAM=None, DATA_PRESET=dict(PRESET))


@pytest.mark.parametrize("aug", [False, True])
def test_real_batcher_mesh_queries_vs_the_float64_chain(tree, hand, tmp_path, monkeypatch, aug):
    from artiboost_amd.realdata import RealBatcher
    from artiboost_amd.synth import ManoLayerHIP
    monkeypatch.chdir(tmp_path)
    ds = _ds(tree)
    on = RealBatcher(ds, PRESET, aug=aug, compute_dtype=torch.float32, seed=3, mesh_queries=N_MESH, mano=ManoLayerHIP(hand))
    off = RealBatcher(ds, PRESET, aug=aug, compute_dtype=torch.float32, seed=3)
    idxs = [0, 4, 8, 5, 2]
    draws = on.draw(len(idxs)) if aug else None
    a, b = on.batch(idxs, draws), off.batch(idxs, draws)
    assert set(a) - set(b) == {"obj_verts_can", "obj_verts_3d", "hand_verts_3d"}
    for k in b:                                                           # every other key: the batch without the argument, bit for bit
        assert torch.equal(a[k], b[k]), k
    assert a["obj_verts_can"].shape == a["obj_verts_3d"].shape == (5, N_MESH, 3) and a["hand_verts_3d"].shape == (5, 778, 3)
    # the float64 chain of DESIGN.md section 22, per sample
    anns = [ds.get_annots(i) for i in idxs]
    table, _ = ds.mesh_vertex_table(N_MESH)
    worst = [0.0, 0.0]
    for s, i in enumerate(idxs):
        m = ds.get_mesh_annots(i)
        rot = draws["rot"][s] if aug else 0.0
        rm = np.array([[np.cos(rot), -np.sin(rot), 0], [np.sin(rot), np.cos(rot), 0], [0, 0, 1]]).astype(np.float32).astype(np.float64)
        root = a["root_joint"][s].cpu().double().numpy()
        np.testing.assert_array_equal(a["obj_verts_can"][s].cpu().numpy(), table[m["table_row"]])
        Tb = np.asarray(anns[s]["obj_transf"], np.float64)
        can = table[m["table_row"]].astype(np.float64)
        want_o = (can @ Tb[:3, :3].T + Tb[:3, 3]) @ rm.T - root
        v = po.mano_lbs(hand, m["hand_pose"][None].astype(np.float64), m["hand_shape"][None].astype(np.float64))[0][0]
        want_h = ((v + m["hand_tsl"].astype(np.float64)) @ E.T) @ rm.T - root
        worst[0] = max(worst[0], np.abs(a["obj_verts_3d"][s].cpu().double().numpy() - want_o).max())
        worst[1] = max(worst[1], np.abs(a["hand_verts_3d"][s].cpu().double().numpy() - want_h).max())
        # ... and the same chain on the canonical corners is the batch's own CORNERS_3D
        want_c = (np.asarray(anns[s]["corners_can"], np.float64) @ Tb[:3, :3].T + Tb[:3, 3]) @ rm.T - root
        assert np.abs(want_c - a["corners_3d"][s].cpu().double().numpy()).max() <= 2e-6
    print(f"\naug={aug}: max err obj_verts_3d {worst[0]:.3e} hand_verts_3d {worst[1]:.3e}")
    assert worst[0] <= BOUND_MANO + BOUND_3D and worst[1] <= BOUND_MANO + BOUND_3D, worst
    again = on.batch(idxs, draws)
    assert all(torch.equal(again[k], a[k]) for k in ("obj_verts_can", "obj_verts_3d", "hand_verts_3d"))


# ------------------------------------------------------------------------------------------------ MixedLoader
def _mixed(tree, B, synth_len, cdt=torch.float32, **kw):
    """MixedLoader over the miniature tree (9 real frames) and a synthetic epoch of synth_len samples, both halves with N_MESH queries."""
    import yaml
    from artiboost_amd.assets import SceneAssets
    from artiboost_amd.realdata import MixedLoader, RealBatcher
    from artiboost_amd.synth import ArtiBoostLoader
    if not _ASSETS:
        _ASSETS.append(SceneAssets("HO3D", seed=1))
    cfg = yaml.safe_load(open(FUSED_CFG))
    ds = _ds(tree)
    _seed(5)
    n_synth = MixedLoader.n_synth_for(B, len(ds), synth_len)
    synth = ArtiBoostLoader.from_assets(_ASSETS[0], dict(cfg["MANAGER"], MESH_QUERIES=N_MESH, EPOCH=1), PRESET, n_synth, synth_len, device="cuda",
                                        compute_dtype=cdt, random_seed=1)
    synth.prepare()
    real = RealBatcher(ds, PRESET, aug=True, compute_dtype=cdt, seed=2, mesh_queries=N_MESH, mano=synth.mano)
    return MixedLoader(real, synth, B, seed=4, **kw)


MESH_KEYS = ("obj_verts_can", "obj_verts_3d", "hand_verts_3d")


def test_mixed_loader_carries_the_mesh_queries_of_both_halves(tree, tmp_path, monkeypatch):
    from artiboost_amd.realdata import RealBatcher, ThreadedPrefetcher
    monkeypatch.chdir(tmp_path)
    ml = _mixed(tree, 4, 8)
    assert (ml.n_real, ml.n_synth) == (2, 2) and len(ml) == 4
    own = [{k: v.clone() for k, v in b.items() if torch.is_tensor(v)} for b in ml]
    assert len(own) == 4
    twin = RealBatcher(ml.real.src, PRESET, aug=True, compute_dtype=torch.float32, seed=2, mesh_queries=N_MESH, mano=ml.synth.mano)
    static = ml.synth.new_static_batch()
    for bi, b in enumerate(own):
        assert b["is_synth"].tolist() == [False, False, True, True]
        for k, last in zip(MESH_KEYS, (N_MESH, N_MESH, 778)):
            assert b[k].shape == (4, last, 3) and b[k].dtype == torch.float32 and torch.isfinite(b[k]).all()
        rb = twin.batch(b["sample_idx"][:2].tolist())                     # the same draws: the twin's generator advances as the loader's did
        assert torch.equal(rb["joints_3d"], b["joints_3d"][:2])
        ml.synth.load_batch(static, bi)
        ml.synth.mesh_queries_into(static)
        for k in MESH_KEYS:
            assert torch.equal(b[k][:2], rb[k]), (bi, k)
            assert torch.equal(b[k][2:], static[k]), (bi, k)
    # the worker thread two batches ahead on its own stream: the loader's own batches, bit for bit
    ml2 = _mixed(tree, 4, 8)
    n = 0
    for b, ref in zip(ThreadedPrefetcher(ml2, depth=2), own):
        for k, v in ref.items():
            assert torch.equal(b[k], v), (n, k)
        n += 1
    assert n == 4
    # the real-only path (after the synthetic share is shut down) yields the real half's queries unchanged
    ml2.synth.synth_shutdown()
    ml2.update()
    assert ml2.n_synth == 0
    b = next(iter(ml2))
    assert b["obj_verts_can"].shape == (4, N_MESH, 3) and b["hand_verts_3d"].shape == (4, 778, 3) and not b["is_synth"].any()


# ------------------------------------------------------------------------------------------------ HoNet
ARCH = {"TYPE": "HoNet", "PRETRAINED": "", "PREVIOUS": [], "OBJ_TRANS_FACTOR": 100, "OBJ_SCALE_FACTOR": 0.0001,
        "BACKBONE": {"TYPE": "ResNet18", "PRETRAINED": False, "FREEZE_BATCHNORM": False},
        "HEAD": {"TYPE": "ManoBranch", "MANO_ASSETS_ROOT": "assets/mano_v1_2", "INPUT_DIM": 512, "NCOMPS": 15, "USE_PCA": True, "USE_SHAPE": True}}


def _model(fused):
    import artiboost_amd.honet  # noqa: F401  (registers HoNet)
    from artiboost_amd import registry as R
    from artiboost_amd.models import Arch
    from artiboost_amd.netutils import build_optimizer
    arch = dict(ARCH, DEVICE="cuda", COMPUTE_DTYPE="f32", INIT_SEED=1, **({"FUSED_MESH_STEP": True} if fused else {}))
    model = Arch({"ARCH": arch}, R.build_arch_model_list(arch, preset_cfg=PRESET))
    opt = build_optimizer(model.models_params, OPTIMIZER="adam", LR=3e-4, WEIGHT_DECAY=0)
    opt.max_norm = 1.0
    return model, opt


def _criterion():
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    cfgc = [{"TYPE": "ManoLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_HAND_VERTS_3D": 1.0, "LAMBDA_SHAPE_REG": 5.0e-7, "LAMBDA_POSE_REG": 5.0e-6},
            {"TYPE": "ObjLoss", "LAMBDA_OBJ_VERTS_3D": 1.0}]
    return Criterion({"LAMBDAS": [1.0, 1.0]}, R.build_criterion_loss_list(cfgc, preset_cfg={}, LAMBDAS=[1.0, 1.0]))


def test_honet_forward_on_a_real_only_batch(tree, hand, tmp_path, monkeypatch):
    from artiboost_amd.realdata import RealBatcher
    from artiboost_amd.synth import ManoLayerHIP
    monkeypatch.chdir(tmp_path)
    _seed(3)
    model, _ = _model(False)
    model.eval()
    rb = RealBatcher(_ds(tree, "test"), PRESET, aug=False, compute_dtype=torch.float32, seed=1, mesh_queries=N_MESH, mano=ManoLayerHIP(hand))
    batch = rb.batch([0, 1, 2, 3])
    with torch.no_grad():
        pd = model(batch)["HoNet"]
    assert pd["obj_verts_3d_abs"].shape == (4, N_MESH, 3) and torch.isfinite(pd["obj_verts_3d_abs"]).all()
    assert torch.isfinite(pd["hand_verts_3d_abs"]).all()


def test_fused_graph_step_over_mixed_batches_equals_the_eager_fused_step(tree, tmp_path, monkeypatch):
    from artiboost_amd.train import TrainStep
    monkeypatch.chdir(tmp_path)
    ml = _mixed(tree, 4, 27)
    assert (ml.n_real, ml.n_synth) == (1, 3) and len(ml) >= 5
    batches = []
    for b in ml:
        batches.append({k: (v.clone() if torch.is_tensor(v) else v) for k, v in b.items()})
        if len(batches) == 5:
            break
    runs = {}
    for graph in (False, True):
        _seed(11)
        model, opt = _model(True)
        model.train()
        ts = TrainStep(model, _criterion(), opt, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batches[0].items()}, use_graph=graph,
                       renderer=None)
        assert ts.fused is not None and ts.mesh and not ts.mesh_queries and ts.use_graph == graph
        assert ts.fused.key_slots["obj_verts_3d_loss"] is not None and ts.fused.key_slots["hand_verts_3d_loss"] is not None
        _seed(17)
        seq = []
        for b in batches:
            ts(b)
            seq.append((ts.hb.store.flat.detach().clone(), ts.fused.out["losses"].clone()))
        runs[graph] = seq
    for i, (a, b) in enumerate(zip(runs[False], runs[True])):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (i, (a[0] - b[0]).abs().max().item(), a[1], b[1])
    assert torch.isfinite(runs[True][-1][1]).all() and not torch.equal(runs[True][0][0], runs[True][4][0])
    assert float(runs[True][0][1][3]) > 0 and float(runs[True][0][1][4]) > 0        # the hand-vertex and object-vertex terms are live


# ------------------------------------------------------------------------------------------------ the script
def test_train_script_with_the_fused_honet_config_on_a_tree_with_real_frames(tmp_path):
    import yaml
    data = tmp_path / "data"
    T.build(str(data), seed=7)
    cfg = yaml.safe_load(open(FUSED_CFG))
    assert cfg["ARCH"]["FUSED_MESH_STEP"] is True and cfg["MANAGER"]["MESH_QUERIES"] > 0
    cfg["TRAIN"]["EPOCH"] = 1
    cfg["DATASET"]["TRAIN"]["DATA_ROOT"] = cfg["DATASET"]["TEST"]["DATA_ROOT"] = str(data)
    cfg["DATA_PRESET"].update(USE_CACHE=True, FILTER_NO_CONTACT=False, FILTER_THRESH=0.0)
    y = tmp_path / "cfg.yaml"
    y.write_text(yaml.dump(cfg))
    cmd = [sys.executable, os.path.join(ROOT, "train", "train_artiboost.py"), "--cfg", str(y), "--gpu_id", "0", "--gpu_render_id", "0",
           "--batch_size", "8", "--exp_id", "rm", "--snapshot", "1", "--synth_len", "8", "--size", "128", "--test_freq", "1", "--workers", "4"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("epoch ")]
    assert len(lines) == 1 and "4 real + 4 synthetic per batch of 8" in lines[-1] and "final_loss" in lines[-1], out.stdout[-2000:]
    tests_ = [l for l in out.stdout.splitlines() if l.startswith("test ")]
    assert len(tests_) == 1 and "5 frames of DATASET.TEST (HO3D)" in tests_[0], out.stdout[-2000:]
    cache = sorted(os.listdir(tmp_path / "common" / "cache" / "HO3D"))
    assert sum(f.endswith(".mano.ab.pkl") for f in cache) == 2 and len(cache) == 4, cache      # train and test split, two files each
    exp = [d for d in os.listdir(tmp_path / "exp") if d.startswith("rm_")]
    sd = torch.load(tmp_path / "exp" / exp[0] / "checkpoints" / "checkpoint" / "HoNet.pth.tar", map_location="cpu", weights_only=False)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.dtype.is_floating_point)
