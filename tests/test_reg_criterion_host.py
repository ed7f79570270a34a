"""The fused regbased criterion and HOPRegNet's FUSED_STEP route, the parts that need no GPU: the C ABI entry point and its dispatcher op,
what FusedRegCriterion accepts and refuses, the layout of its loss vector, and FUSED_STEP being opt-in."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "artiboost_hip.h")

MANO = {"TYPE": "ManoLoss", "LAMBDA_JOINTS_3D": 0.0, "LAMBDA_HAND_VERTS_3D": 0.0, "LAMBDA_SHAPE_REG": 5.0e-7, "LAMBDA_POSE_REG": 5.0e-6}
JOINTS = {"TYPE": "JointsLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_CORNERS_3D": 0.2}


def _crit(cfgc, lambdas):
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    return Criterion({"LAMBDAS": lambdas}, R.build_criterion_loss_list(cfgc, preset_cfg={}, LAMBDAS=lambdas))


def test_header_declares_reg_pose_loss_and_the_libraries_export_it():
    txt = open(HEADER).read()
    assert re.search(r"\bint\s+ab_reg_pose_loss\s*\(", txt) and re.search(r"@check\s+ab_reg_pose_loss:", txt)
    from artiboost_amd import _lib, gen_torch_ops
    assert hasattr(_lib.cdll(), "ab_reg_pose_loss")
    gen = open(os.path.join(ROOT, "artiboost_amd", "csrc", "torch_ops_gen.cpp")).read()
    assert 'm.impl("reg_pose_loss", &w_reg_pose_loss);' in gen and "reg_pose_loss(Tensor? joints_pred" in gen
    c = gen_torch_ops.contracts()["ab_reg_pose_loss"]
    assert any(cl.startswith("strided:") and "g_transf" in cl for cl in c) and any("weights12_host" in cl for cl in c)
    params = {n: p for _, n, p in gen_torch_ops.declarations()}["ab_reg_pose_loss"]
    assert params[-1] == ("void*", "stream") and [pn for _, pn in params[:5]] == ["joints_pred", "mano_pca_pose", "mano_shape", "transf", "transf_stride"]


def test_fused_reg_criterion_accepts_the_shipped_list_and_lays_out_its_vector():
    from artiboost_amd.criterions import FusedRegCriterion
    f = FusedRegCriterion(_crit([MANO, JOINTS, {"TYPE": "HandOrdLoss"}, {"TYPE": "SceneOrdLoss"}], [1.0, 1.0, 0.1, 0.1]), 15)
    assert len(f.LOSS_KEYS) == f.LOSS_WIDTH == 16
    assert f.LOSS_KEYS[:6] == ("joints_3d_loss", "corners_3d_loss", "joint_ord_loss", "part_ord_loss", "scene_ord_loss", "final_loss")
    assert f.LOSS_KEYS[8:10] == ("mano_shape", "mano_pca_pose") and f.LOSS_KEYS[6] is None and f.LOSS_KEYS[10] is None
    # JointsLoss's joints_3d_loss overwrites ManoLoss's entry of the same name; switched-off terms are None
    assert f.key_slots["joints_3d_loss"] == 0 and f.key_slots["hand_verts_3d_loss"] is None
    assert list(f.weights) == pytest.approx([1.0, 0.2, 1.0, 1.0, 1.0, 1.0, 0.1, 0.1, 5e-7, 5e-6, 0.0, 1.0], rel=1e-6)
    # ManoLoss alone, with its joint term: the entry is ManoLoss's own
    g = FusedRegCriterion(_crit([dict(MANO, LAMBDA_JOINTS_3D=2.0)], [1.0]), 45)
    assert g.key_slots["joints_3d_loss"] == 10 and g.LOSS_KEYS[10] == "joints_3d_loss" and g.LOSS_KEYS[0] is None
    # a JointsLoss with its joint term off reports None under that name, as the registry route does
    h = FusedRegCriterion(_crit([dict(MANO, LAMBDA_JOINTS_3D=2.0), dict(JOINTS, LAMBDA_JOINTS_3D=0.0)], [1.0, 1.0]), 15)
    assert h.key_slots["joints_3d_loss"] is None


def test_fused_reg_criterion_refuses_what_the_kernel_does_not_compute():
    from artiboost_amd.criterions import FusedRegCriterion
    with pytest.raises(NotImplementedError):
        FusedRegCriterion(_crit([JOINTS, {"TYPE": "HandOrdLoss"}, {"TYPE": "SceneOrdLoss"}], [0.5, 0.2, 0.1]), 15)
    info = {str(i + 1): {} for i in range(21)}
    with pytest.raises(NotImplementedError):
        FusedRegCriterion(_crit([MANO, JOINTS, {"TYPE": "SymCornerLoss", "LAMBDA_SYM_CORNERS_3D": 0.7, "MODEL_INFO": info}], [1.0, 1.0, 0.3]), 15)
    verts = _crit([dict(MANO, LAMBDA_HAND_VERTS_3D=1.0), JOINTS], [1.0, 1.0])
    FusedRegCriterion(verts, 15, {"joints_3d": torch.zeros(2, 21, 3)})            # no such target in the batch: the registry loss skips the term too
    with pytest.raises(NotImplementedError):
        FusedRegCriterion(verts, 15, {"joints_3d": torch.zeros(2, 21, 3), "hand_verts_3d": torch.zeros(2, 778, 3)})
    FusedRegCriterion(_crit([MANO, JOINTS], [1.0, 1.0]), 15, {"hand_verts_3d": torch.zeros(2, 778, 3)})      # zero lambda: nothing to compute


def test_fused_step_is_opt_in_and_the_shipped_configs_say_so():
    import yaml
    base = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_regbased_artiboost_mi355x.yaml")))
    fused = yaml.safe_load(open(os.path.join(ROOT, "config", "ho3dv2_regbased_artiboost_mi355x_fused.yaml")))
    assert "FUSED_STEP" not in base["ARCH"] and fused["ARCH"].pop("FUSED_STEP") is True
    assert fused == base
    # TrainStep reads the key from the model: without it the route is today's (no fused criterion, no graphs)
    from artiboost_amd.train import TrainStep

    class Store:
        device = torch.device("cpu")

    class Model:
        HAS_BOX_HEAD, store, ncomps, inp_res, center_idx = False, Store(), 15, [64, 64], 0

    class ArchStub:
        models = {"HOPRegNet": {"id": 0}}

        def __init__(self, m):
            self.model_list = [m]

    crit = _crit([MANO, JOINTS, {"TYPE": "HandOrdLoss"}, {"TYPE": "SceneOrdLoss"}], [1.0, 1.0, 0.1, 0.1])
    batch = {"root_joint": torch.zeros(2, 3)}
    ts = TrainStep(ArchStub(Model()), crit, None, batch, use_graph=True)
    assert ts.fused is None and not ts.use_graph and not ts.split and not ts.reg

    class FusedModel(Model):
        FUSED_STEP = True

    ts = TrainStep(ArchStub(FusedModel()), crit, None, batch, use_graph=False)
    assert type(ts.fused).__name__ == "FusedRegCriterion" and ts.reg and not ts.split
    # a loss outside the kernel: back to the registry losses, eagerly
    info = {str(i + 1): {} for i in range(21)}
    sym = _crit([MANO, JOINTS, {"TYPE": "SymCornerLoss", "LAMBDA_SYM_CORNERS_3D": 0.7, "MODEL_INFO": info}], [1.0, 1.0, 0.3])
    ts = TrainStep(ArchStub(FusedModel()), sym, None, batch, use_graph=True)
    assert ts.fused is None and not ts.use_graph
