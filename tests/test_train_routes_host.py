"""TrainStep's route decision table, on the CPU: which fused criterion, whether the step is graph-replayed, split, pipelined, and the
public booleans, for every (model declaration x criterion x fused_criterion x pipeline_render x AB_DDP_SPLIT).  The expected values were
recorded from the TrainStep that held all of these decisions in one `if` ladder; they are literals, not computed from the code under test."""
import itertools

import pytest
import torch

MANO = {"TYPE": "ManoLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_HAND_VERTS_3D": 0.0, "LAMBDA_SHAPE_REG": 5.0e-7, "LAMBDA_POSE_REG": 5.0e-6}
JOINTS = {"TYPE": "JointsLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_CORNERS_3D": 0.2}
ORD = [{"TYPE": "HandOrdLoss"}, {"TYPE": "SceneOrdLoss"}]
OBJ = {"TYPE": "ObjLoss", "LAMBDA_OBJ_VERTS_3D": 1.0}
CHAMFER = {"TYPE": "ChamferLoss", "LAMBDA_CHAMFER": 1.0}      # in none of the three kernels

# what the model class declares -> (class attributes, a loss list its route's kernel computes)
MODELS = {"nothing": ({}, [JOINTS] + ORD), "no_box_head": ({"HAS_BOX_HEAD": False}, [JOINTS] + ORD),
          "fused_step": ({"HAS_BOX_HEAD": False, "FUSED_STEP": True}, [MANO, JOINTS] + ORD),
          "fused_mesh_step": ({"HAS_BOX_HEAD": False, "FUSED_MESH_STEP": True}, [MANO, OBJ])}
RENDER = (False, True, "opt")
SPLIT_ENV = (None, "0", "1")

# (model, criterion fusable, fused_criterion) -> one entry per (pipeline_render, AB_DDP_SPLIT) in the order of RENDER x SPLIT_ENV:
# "<fused criterion class, without Fused...Criterion>:<flags>", flags = the true ones of g use_graph, s split, p pipeline, o pipeline_opt,
# r reg, m mesh, q mesh_queries
EXPECTED = {
    ("nothing", True, True): "Pose:g Pose:g Pose:gs Pose:gp Pose:gp Pose:gsp Pose:go Pose:go Pose:gso",
    ("nothing", True, False): "None:g None:g None:g None:gp None:gp None:gp None:go None:go None:go",
    ("nothing", False, True): "None: None: None: None:p None:p None:p None:o None:o None:o",
    ("nothing", False, False): "None:g None:g None:g None:gp None:gp None:gp None:go None:go None:go",
    ("no_box_head", True, True): "None: None: None: None:p None:p None:p None:o None:o None:o",
    ("no_box_head", True, False): "None: None: None: None:p None:p None:p None:o None:o None:o",
    ("no_box_head", False, True): "None: None: None: None:p None:p None:p None:o None:o None:o",
    ("no_box_head", False, False): "None: None: None: None:p None:p None:p None:o None:o None:o",
    ("fused_step", True, True): "Reg:gr Reg:gr Reg:gr Reg:gpr Reg:gpr Reg:gpr Reg:gor Reg:gor Reg:gor",
    ("fused_step", True, False): "None:r None:r None:r None:pr None:pr None:pr None:or None:or None:or",
    ("fused_step", False, True): "None:r None:r None:r None:pr None:pr None:pr None:or None:or None:or",
    ("fused_step", False, False): "None:r None:r None:r None:pr None:pr None:pr None:or None:or None:or",
    ("fused_mesh_step", True, True): "Mesh:gmq Mesh:gmq Mesh:gmq Mesh:gmq Mesh:gmq Mesh:gmq Mesh:gmq Mesh:gmq Mesh:gmq",
    ("fused_mesh_step", True, False): "None:m None:m None:m None:m None:m None:m None:m None:m None:m",
    ("fused_mesh_step", False, True): "None:m None:m None:m None:m None:m None:m None:m None:m None:m",
    ("fused_mesh_step", False, False): "None:m None:m None:m None:m None:m None:m None:m None:m None:m",
}


class _Store:
    device = torch.device("cpu")


class _Opt:
    def use_device_hyper(self, dev):
        pass

    def advance_hyper(self):
        pass


class _Arch:
    def __init__(self, m, name):
        self.model_list, self.models = [m], {name: {"id": 0}}


class _Renderer:
    """A loader that offers the mesh queries; render_into is never reached at construction."""
    mesh_queries = 4

    def mesh_queries_into(self, static):
        static["hand_verts_3d"] = torch.zeros(2, 778, 3)


def _criterion(cfgc):
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    lambdas = [1.0] * len(cfgc)
    return Criterion({"LAMBDAS": lambdas}, R.build_criterion_loss_list(cfgc, preset_cfg={}, LAMBDAS=lambdas))


def _observe(model, fusable, fused_criterion, render, env, monkeypatch):
    from artiboost_amd.train import TrainStep
    attrs, losses = MODELS[model]
    hb = type("Model", (), dict(attrs, store=_Store(), ncomps=15, inp_res=[64, 64], center_idx=0))()
    if env is None:
        monkeypatch.delenv("AB_DDP_SPLIT", raising=False)
    else:
        monkeypatch.setenv("AB_DDP_SPLIT", env)
    batch = {"root_joint": torch.zeros(2, 3), "joints_3d": torch.zeros(2, 21, 3), "_samples": torch.zeros(2, 8, dtype=torch.uint8),
             "image_nhwc4_padded": torch.zeros(2, 14, 16, 4)}
    ts = TrainStep(_Arch(hb, model), _criterion(losses if fusable else losses + [CHAMFER]), _Opt(), batch, use_graph=True,
                   renderer=_Renderer(), fused_criterion=fused_criterion, pipeline_render=render)
    name = "None" if ts.fused is None else type(ts.fused).__name__[len("Fused"):-len("Criterion")]
    flags = (("g", ts.use_graph), ("s", ts.split), ("p", ts.pipeline), ("o", ts.pipeline_opt), ("r", ts.reg), ("m", ts.mesh),
             ("q", ts.mesh_queries))
    assert all(type(v) is bool for _, v in flags), flags
    # the pipelined modes hold the NEXT batch's render inputs (and, copying, its own image); the others have no second batch
    assert (ts.rstatic is not None) == (ts.pipeline or ts.pipeline_opt)
    if ts.rstatic is not None:
        assert sorted(ts.rstatic) == (["_samples", "image_nhwc4_padded"] if ts.pipeline else ["_samples"])
        assert all(ts.rstatic[k] is not ts.static[k] for k in ts.rstatic)
    return name + ":" + "".join(f for f, v in flags if v)


def test_the_table_covers_every_case():
    assert sorted(EXPECTED) == sorted(itertools.product(MODELS, (True, False), (True, False)))
    assert all(len(row.split()) == len(RENDER) * len(SPLIT_ENV) for row in EXPECTED.values())


@pytest.mark.parametrize("model,fusable,fused_criterion", sorted(EXPECTED))
def test_train_step_decides_as_recorded(model, fusable, fused_criterion, monkeypatch):
    # (a side stream of the pipelined modes is the one device object made at construction)
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: object())
    for k in ("AB_FAKE_COMM", "AB_DDP_SINGLE_RANK"):
        monkeypatch.delenv(k, raising=False)
    got = [_observe(model, fusable, fused_criterion, render, env, monkeypatch) for render in RENDER for env in SPLIT_ENV]
    assert got == EXPECTED[(model, fusable, fused_criterion)].split()
