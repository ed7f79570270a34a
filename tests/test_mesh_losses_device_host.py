"""CPU: the surface of the ChamferLoss / AlignLoss device route -- declared symbols and dispatcher ops, the argument
contracts of ab_chamfer_rigid, the closed form ab_procrustes_loss rests on against the reference's autograd values
(tests/golden/mesh_losses.npz), and TrainStep's refusal to capture a step that holds either loss."""
import os

import numpy as np
import pytest
import torch

NAMES = ("ab_chamfer_rigid", "ab_chamfer_rigid_workspace", "ab_procrustes_loss")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mesh_losses.npz"), allow_pickle=False))


def test_entry_points_are_declared_and_registered():
    from artiboost_amd import _lib as L
    assert set(NAMES) <= set(L.declared_symbols())
    L.lib()
    for n in NAMES:
        assert hasattr(torch.ops.artiboost_hip, n[3:]), n
    assert torch.ops.artiboost_hip.chamfer_rigid_workspace(2, 300, 257) == 2 * (2 + 2) * 16 * 4
    assert torch.ops.artiboost_hip.chamfer_rigid_workspace(0, 300, 257) == 0


def test_chamfer_rigid_op_checks_its_arguments():
    from artiboost_amd import _lib as L
    L.lib()
    op = torch.ops.artiboost_hip.chamfer_rigid
    B, N, M = 2, 5, 7
    z = lambda *s: torch.zeros(*s)      # noqa: E731
    args = [z(B, N, 3), z(B, 9), z(B, 3), z(B, M, 3), z(B, 3), z(B, 8), B, N, M, z(1), None, None, None, None, z(B, 9), z(B, 3), torch.zeros(1 << 12, dtype=torch.uint8)]
    with pytest.raises(RuntimeError, match="must be a HIP tensor"):
        op(*args)
    # The wrapper checks placement before sizes, so the undersized g_rot is refused live in tests/test_gpu_mesh_losses.py; here the clause
    # is pinned where it is written and where it is generated.
    from artiboost_amd import gen_torch_ops
    clauses = gen_torch_ops.contracts()
    assert any(c.replace(" ", "").startswith("rotg_rot>=B*9") for c in clauses["ab_chamfer_rigid"])
    assert any("ab_chamfer_rigid_workspace(B,N,M)" in c for c in clauses["ab_chamfer_rigid"])
    src = open(gen_torch_ops.OUT).read()
    assert 'ck_numel(OP, "g_rot", g_rot, (int64_t)(B*9));' in src and 'ck_numel(OP, "g_pred", g_pred, (int64_t)(B*n*3));' in src


def procrustes_closed_form(pred, targ, root):
    """float64: loss and d loss / d pred of AlignLoss without an SVD backward (R = u v^T is the optimum of the alignment):
    per sample c^2 (1 - s^2) / (3 n) up to the 1e-8 of the norms, here from the residual; d loss / d M = -2 c^2 s R / (3 n B)."""
    pred, xyz = np.asarray(pred, np.float64), np.asarray(targ, np.float64) + np.asarray(root, np.float64)[:, None]
    B, n = pred.shape[:2]
    Xc, Pc = xyz - xyz.mean(1, keepdims=True), pred - pred.mean(1, keepdims=True)
    c = np.sqrt((Xc ** 2).sum((1, 2))) + 1e-8
    p = np.sqrt((Pc ** 2).sum((1, 2))) + 1e-8
    Xh, Ph = Xc / c[:, None, None], Pc / p[:, None, None]
    M = np.einsum("bia,bik->bak", Xh, Ph)
    u, w, vt = np.linalg.svd(M)
    R, s = u @ vt, w.sum(1)
    res = s[:, None, None] * np.einsum("bak,bik->bia", R, Ph) - Xh
    sample = c ** 2 * (res ** 2).sum((1, 2)) / (3 * n)
    # s = tr(R^T M) and R are the optimum, so with q = |Ph|^2 (= 1 up to the 1e-8):  d loss / d Ph_i = k ((2 - q) R^T Xh_i - s Ph_i)
    k, q = -2 * c ** 2 * s / (3 * n * B), (Ph ** 2).sum((1, 2))
    g = k[:, None, None] * ((2 - q)[:, None, None] * np.einsum("bak,bia->bik", R, Xh) - s[:, None, None] * Ph)
    gdot = (g * Ph).sum((1, 2)) * p / (p - 1e-8)                             # through Ph = Pc / (|Pc| + 1e-8): the radial part drops out
    gc = (g - gdot[:, None, None] * Ph) / p[:, None, None]
    return sample.mean(), sample, gc - gc.mean(1, keepdims=True)             # ... and through the centring


def test_procrustes_closed_form_reproduces_the_reference_autograd(golden):
    loss, sample, g = procrustes_closed_form(golden["joints_3d_abs"], golden["joints_3d"], golden["root_joint"])
    np.testing.assert_allclose(loss, golden["procrustes_aligned_loss"], rtol=2e-6)
    ref = golden["g_joints_3d_abs"] / 0.3
    np.testing.assert_allclose(g, ref, rtol=1e-5, atol=2e-6 * np.abs(ref).max())


class _Store:
    device = torch.device("cpu")


class _Opt:
    def use_device_hyper(self, dev):
        pass


class _Arch:
    def __init__(self, m):
        self.model_list, self.models = [m], {"Model": {"id": 0}}


class _NoCuda:
    def __getattr__(self, name):
        raise AssertionError(f"torch.cuda.{name} touched before the refusal")


def test_capture_refuses_the_eager_only_losses_before_touching_the_device(monkeypatch):
    from artiboost_amd import registry as R
    from artiboost_amd.criterions import Criterion
    from artiboost_amd.train import TrainStep
    for k in ("AB_FAKE_COMM", "AB_DDP_SINGLE_RANK", "AB_DDP_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    cfgc = [{"TYPE": "JointsLoss", "LAMBDA_JOINTS_3D": 1.0, "LAMBDA_CORNERS_3D": 0.2}, {"TYPE": "ChamferLoss", "LAMBDA_CHAMFER": 1.0}]
    crit = Criterion({"LAMBDAS": [1.0, 1.0]}, R.build_criterion_loss_list(cfgc, preset_cfg={}, LAMBDAS=[1.0, 1.0]))
    hb = type("Model", (), dict(store=_Store(), ncomps=15, inp_res=[64, 64], center_idx=0))()
    batch = {"root_joint": torch.zeros(2, 3), "joints_3d": torch.zeros(2, 21, 3)}
    ts = TrainStep(_Arch(hb), crit, _Opt(), batch, use_graph=True, fused_criterion=False)
    assert ts.use_graph and ts.fused is None            # the one construction that reaches _capture with such a list
    monkeypatch.setattr(torch, "cuda", _NoCuda())
    with pytest.raises(NotImplementedError, match="eager route only"):
        ts._capture()
    with pytest.raises(NotImplementedError, match="eager route only"):
        ts()
