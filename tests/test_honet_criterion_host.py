"""HoNet's fused mesh criterion and the FUSED_MESH_STEP route, the parts that need no GPU: the two C ABI entry points and their dispatcher
ops, what FusedMeshCriterion accepts and refuses, the layout of its loss vector against the registry route's dict, and the new key being
opt-in and confined to its own config."""
import glob
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "artiboost_hip.h")

MANO = {"TYPE": "ManoLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_HAND_VERTS_3D": 1.0, "LAMBDA_SHAPE_REG": 5.0e-7, "LAMBDA_POSE_REG": 5.0e-6}
OBJ = {"TYPE": "ObjLoss", "LAMBDA_OBJ_VERTS_3D": 1.0}


def _crit(cfgc, lambdas):
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    return Criterion({"LAMBDAS": lambdas}, R.build_criterion_loss_list(cfgc, preset_cfg={}, LAMBDAS=lambdas))


def _cpu_batch(B=2, N=5):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: 0.05 * torch.randn(*s, generator=g)      # noqa: E731
    preds = {"joints_3d_abs": r(B, 21, 3), "hand_verts_3d_abs": r(B, 778, 3), "obj_verts_3d_abs": r(B, N, 3), "mano_shape": r(B, 10),
             "mano_pca_pose": r(B, 18)}
    targs = {"root_joint": r(B, 3), "joints_3d": r(B, 21, 3), "hand_verts_3d": r(B, 778, 3), "obj_verts_3d": r(B, N, 3)}
    return preds, targs


def test_header_declares_both_entry_points_and_the_libraries_export_them():
    txt = open(HEADER).read()
    from artiboost_amd import _lib, gen_torch_ops
    gen = open(os.path.join(ROOT, "artiboost_amd", "csrc", "torch_ops_gen.cpp")).read()
    cons = gen_torch_ops.contracts()
    decl = {n: p for _, n, p in gen_torch_ops.declarations()}
    for name in ("ab_mesh_queries", "ab_honet_loss"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt) and re.search(r"@check\s+%s:" % name, txt), name
        assert hasattr(_lib.cdll(), name), name
        assert 'm.impl("%s", &w_%s);' % (name[3:], name[3:]) in gen, name
        assert name in cons and decl[name][-1] == ("void*", "stream")
    assert any(cl.startswith("bytes samples") for cl in cons["ab_mesh_queries"])
    assert any("weights7_host" in cl for cl in cons["ab_honet_loss"]) and any("workspace" in cl for cl in cons["ab_honet_loss"])
    assert [pn for _, pn in decl["ab_honet_loss"][:4]] == ["joints_3d_abs", "hand_verts_3d_abs", "obj_verts_3d_abs", "corners_3d_abs"]
    assert ("const uint8_t*", "samples") in decl["ab_mesh_queries"] and ("const int64_t*", "obj_id") in decl["ab_mesh_queries"]
    # the chunk / workspace queries run on the host: one row of 8 floats per (sample, object chunk + the hand block)
    lib = _lib.cdll()
    chunk = next(n for n in range(1, 1 << 16) if lib.ab_honet_loss_chunks(n + 1) == 2)
    assert lib.ab_honet_loss_chunks(0) == 0 and lib.ab_honet_loss_chunks(1) == 1 and lib.ab_honet_loss_chunks(chunk) == 1
    assert lib.ab_honet_loss_workspace(3, chunk + 1) == 3 * 3 * 8 * 4 and lib.ab_honet_loss_workspace(3, 0) == 3 * 8 * 4


def test_fused_mesh_criterion_accepts_mano_alone_and_mano_plus_obj():
    from artiboost_amd.criterions import FusedMeshCriterion
    preds, targs = _cpu_batch()
    for cfgc, lambdas in (([MANO], [1.0]), ([MANO, OBJ], [1.0, 0.5])):
        crit = _crit(cfgc, lambdas)
        f = FusedMeshCriterion(crit, 15, targs)
        _, ref = crit.compute_losses(preds, targs)
        # LOSS_KEYS: exactly the registry dict's keys (final_loss is one of them), each once
        named = [k for k in f.LOSS_KEYS if k is not None]
        assert len(f.LOSS_KEYS) == f.LOSS_WIDTH == 8 and sorted(named) == sorted(ref) == sorted(f.key_slots) and len(set(named)) == len(named)
        assert list(f.key_slots) == list(ref)                      # ... in the registry's own order
        assert f.LOSS_KEYS[5] == "final_loss" and f.LOSS_KEYS[6] is None and f.LOSS_KEYS[7] is None
        assert f.draw(torch.device("cpu")) is None
    assert list(f.weights) == pytest.approx([5e-7, 5e-6, 1.0, 1.0, 1.0, 1.0, 0.5], rel=1e-6)
    assert list(FusedMeshCriterion(_crit([MANO], [2.0]), 15).weights) == pytest.approx([5e-7, 5e-6, 1.0, 1.0, 0.0, 2.0, 0.0], rel=1e-6)


def test_switched_off_terms_and_absent_targets_are_none_as_on_the_registry_route():
    from artiboost_amd.criterions import FusedMeshCriterion
    preds, targs = _cpu_batch()
    cases = [([dict(MANO, LAMBDA_HAND_VERTS_3D=0.0, LAMBDA_SHAPE_REG=0.0), OBJ], targs),
             ([MANO, OBJ], {k: v for k, v in targs.items() if k not in ("hand_verts_3d", "obj_verts_3d")}),
             ([MANO, dict(OBJ, LAMBDA_OBJ_VERTS_3D=0.0)], {k: v for k, v in targs.items() if k != "joints_3d"})]
    for cfgc, t in cases:
        crit = _crit(cfgc, [1.0, 1.0])
        _, ref = crit.compute_losses(preds, t)
        f = FusedMeshCriterion(crit, 15, t)
        assert {k for k, s in f.key_slots.items() if s is None} == {k for k, v in ref.items() if v is None}
        assert sorted(k for k in f.LOSS_KEYS if k is not None) == sorted(k for k, v in ref.items() if v is not None)


def test_fused_mesh_criterion_refuses_what_the_kernel_does_not_compute():
    from artiboost_amd.criterions import FusedMeshCriterion
    joints = {"TYPE": "JointsLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_CORNERS_3D": 0.2}
    for cfgc in ([MANO, joints], [MANO, OBJ, joints], [MANO, {"TYPE": "ChamferLoss", "LAMBDA_CHAMFER": 1.0}], [OBJ], [OBJ, MANO], [MANO, MANO]):
        with pytest.raises(NotImplementedError):
            FusedMeshCriterion(_crit(cfgc, [1.0] * len(cfgc)), 15)


def test_fused_mesh_step_is_opt_in_and_only_its_own_config_sets_it():
    import yaml
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_mi355x.yaml")))
    fused = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_honet_mi355x_fused.yaml")))
    assert "FUSED_MESH_STEP" not in base["ARCH"] and fused["ARCH"].pop("FUSED_MESH_STEP") is True
    assert fused == base
    for path in glob.glob(os.path.join(ROOT, "config", "*.yaml")):
        if os.path.basename(path) != "ho3dv2_honet_mi355x_fused.yaml":
            assert "FUSED_MESH_STEP" not in open(path).read(), path
    # TrainStep reads the key from the model: without it HoNet's route is the eager one
    from artiboost_amd.train import TrainStep

    class Store:
        device = torch.device("cpu")

    class Model:
        HAS_BOX_HEAD, store, ncomps, inp_res, center_idx = False, Store(), 15, [64, 64], 0

    class ArchStub:
        models = {"HoNet": {"id": 0}}

        def __init__(self, m):
            self.model_list = [m]

    crit = _crit([MANO, OBJ], [1.0, 1.0])
    batch = {"root_joint": torch.zeros(2, 3), "joints_3d": torch.zeros(2, 21, 3)}
    ts = TrainStep(ArchStub(Model()), crit, None, batch, use_graph=True)
    assert ts.fused is None and not ts.use_graph and not ts.mesh and not ts.mesh_queries

    class FusedModel(Model):
        FUSED_MESH_STEP = True

    ts = TrainStep(ArchStub(FusedModel()), crit, None, batch, use_graph=False, pipeline_render="opt", renderer=object())
    assert type(ts.fused).__name__ == "FusedMeshCriterion" and ts.mesh and not ts.reg and not ts.split and not ts.pipeline_opt
    assert ts.fused.key_slots["joints_3d_loss"] == 2 and ts.fused.key_slots["obj_verts_3d_loss"] is None and not ts.mesh_queries
    # a loss outside the kernel: back to the registry losses, eagerly
    other = _crit([MANO, {"TYPE": "JointsLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_CORNERS_3D": 0.2}], [1.0, 1.0])
    ts = TrainStep(ArchStub(FusedModel()), other, None, batch, use_graph=True)
    assert ts.fused is None and not ts.use_graph
