"""The hand-mesh fit of the submission pass, the parts that need no GPU: the float64 oracle of ab_mano_fit (its MANO layer against
the reference's own layer output, its gradient against finite differences, its quaternion conversion, its Adam against a worked
example), IKNet's checkpoint format and BatchNorm fold, and the CodaLab dump of HOSubmitEpochPass with the fitter stubbed."""
import json
import os

import numpy as np
import pytest
import torch

import fit_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand():
    from artiboost_amd.hpregnet import load_hand_model
    return load_hand_model(None)


def _state(B, seed, dtype=torch.float64):
    """Seeded raw quaternions [B,64] and predicted joints [B,21,3] (a hand-sized random skeleton around a root)."""
    g = torch.Generator().manual_seed(seed)
    quat = torch.randn(B, 64, generator=g, dtype=dtype)
    quat.view(B, 16, 4)[:, :, 0] += 2.0
    pj = 0.03 * torch.randn(B, 21, 3, generator=g, dtype=dtype) + torch.tensor([0.0, 0.0, 0.6], dtype=dtype)
    return quat, pj


def test_oracle_mano_matches_the_reference_layer_golden(golden_dir):
    """tests/golden/mano.npz holds the reference's own JAX MANO layer (manolayer.py, flat hand mean) on the seeded stand-in hand,
    wrist-relative; the oracle's layer is centred on joint 9 -- the same up to that translation."""
    from artiboost_amd.assets import make_hand_model
    g = np.load(os.path.join(golden_dir, "mano.npz"))
    mano = fo.Mano(make_hand_model(int(g["hand_model_seed"])))
    v, j = mano(torch.from_numpy(g["pose"]), torch.from_numpy(g["betas"]))
    np.testing.assert_allclose((v - j[:, :1]).numpy(), g["verts_rel_wrist"], rtol=0, atol=1e-9)
    np.testing.assert_allclose((j - j[:, :1]).numpy(), g["joints_rel_wrist"], rtol=0, atol=1e-9)
    assert float(j[:, 9].abs().max()) == 0.0


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mano_fit.npz"))


def test_iknet_and_quaternion_conversion_match_the_reference(golden_dir):
    """tests/golden/mano_fit.npz: the reference's IKNet (model.py + utils.py, float64) on seeded weights; this build's IKNet class
    (same keys, same init order) gives the same raw quaternions, and the oracle's conversion gives the reference's so3."""
    import gen_mano_fit_golden as gen
    from artiboost_amd.fitting import IKNet
    g = _golden(golden_dir)
    net = gen.seeded_iknet(IKNet)
    with torch.no_grad():
        q = net(torch.from_numpy(g["iknet_in"]))
    qn = torch.nn.functional.normalize(q, p=2, dim=-1, eps=1e-12)
    np.testing.assert_allclose(qn.numpy(), g["iknet_quat"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(fo.quat_to_aa(q).reshape(-1, 48).numpy(), g["iknet_so3"], rtol=0, atol=1e-11)


def test_oracle_objective_matches_the_reference_residuals(golden_dir):
    """`residuals` of fittingunit.py (float64 under the numpy shim) at 16 points: the oracle's value, and its autograd gradient
    against the reference's central differences (points away from the |.| and clip kinks)."""
    g = _golden(golden_dir)
    mano = fo.Mano(_hand())
    x = torch.from_numpy(g["params"])
    so3_init, root, target = (torch.from_numpy(g[k]) for k in ("so3_init", "root", "target"))
    grad, err = fo.grad(x, so3_init, root, target, mano)
    np.testing.assert_allclose(err.numpy(), g["residuals"], rtol=1e-10, atol=0)
    scale = np.abs(g["fd_grad"]).max(1, keepdims=True)
    np.testing.assert_allclose(grad.numpy(), g["fd_grad"], rtol=0, atol=1e-6 * scale.max())
    assert (np.abs(grad.numpy() - g["fd_grad"]) <= 1e-5 * scale).all()


def test_oracle_mesh_matches_the_reference_mano_de(golden_dir):
    g = _golden(golden_dir)
    mano = fo.Mano(_hand())
    v, j = fo.mano_de(torch.from_numpy(g["params"]), torch.from_numpy(g["root"]), torch.from_numpy(g["bone"]), mano)
    np.testing.assert_allclose(v.numpy(), g["mano_de_verts"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(j.numpy(), g["mano_de_joints"], rtol=0, atol=1e-12)


def test_adam_matches_a_hand_worked_two_step_example():
    """jax.experimental.optimizers.adam(0.03, b1=0.5, b2=0.5), eps 1e-8, step index i = n: bias correction 1 - 0.5^(n+1)."""
    x = torch.tensor([1.0], dtype=torch.float64)
    m = v = torch.zeros(1, dtype=torch.float64)
    x, m, v = fo.adam_step(x, torch.tensor([2.0], dtype=torch.float64), m, v, 1)
    # m = 1, v = 2; mhat = 1 / 0.75, vhat = 2 / 0.75
    x1 = 1.0 - 0.03 * (4.0 / 3.0) / (np.sqrt(8.0 / 3.0) + 1e-8)
    assert (float(m), float(v)) == (1.0, 2.0) and abs(float(x) - x1) < 1e-15
    x, m, v = fo.adam_step(x, torch.tensor([-4.0], dtype=torch.float64), m, v, 2)
    # m = -2 + 0.5 = -1.5, v = 8 + 1 = 9; mhat = -1.5 / 0.875, vhat = 9 / 0.875
    x2 = x1 + 0.03 * (1.5 / 0.875) / (np.sqrt(9.0 / 0.875) + 1e-8)
    assert (float(m), float(v)) == (-1.5, 9.0) and abs(float(x) - x2) < 1e-15


def test_pose_regulariser_pulls_towards_the_batch_mean():
    """reg = mean over [B,48] of (so3 - so3_init)^2: the gradient is 0.02 / 48 (so3 - mean_b so3_init_b), whatever hand it is."""
    hm = _hand()
    quat, pj = _state(5, seed=8)
    mano = fo.Mano(hm)
    so3_init, root, bone, target = fo.prepare(quat, pj)
    x = torch.cat([so3_init, torch.zeros(5, 10, dtype=torch.float64), bone[:, None]], 1)
    g_all, _ = fo.grad(x, so3_init, root, target, mano)
    g_own, _ = fo.grad(x, so3_init[:1].expand(5, 48), root, target, mano)      # as if every hand's batch were hand 0 alone
    d = (g_all - g_own)[:, :48]
    np.testing.assert_allclose(d.numpy(), (0.02 / 48 * (so3_init[:1] - so3_init.mean(0, keepdim=True))).expand(5, 48).numpy(),
                               rtol=1e-9, atol=1e-15)


# ------------------------------------------------------------------------------------------------ IKNet weights
def test_iknet_checkpoint_format_and_the_batchnorm_fold(tmp_path):
    from artiboost_amd.fitting import IKNet, fold_iknet, load_iknet_checkpoint
    torch.manual_seed(0)
    net = IKNet()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.uniform_(-0.5, 0.5)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.uniform_(-0.2, 0.2)
    sd = dict(net.state_dict())
    sd["mano_layer.th_betas"] = torch.zeros(1, 10)        # CheckpointIO drops every key naming mano_layer
    path = tmp_path / "iknet.pt"
    torch.save({"model": sd}, path)
    loaded = load_iknet_checkpoint(str(path))
    assert not any("mano_layer" in k for k in loaded)
    net2 = IKNet()
    net2.load_state_dict(loaded)                         # strict: exactly the reference's keys
    net2.eval()
    x = torch.randn(9, 21, 3)
    with torch.no_grad():
        ref = net2(x).reshape(9, 64).double()
    h = torch.cat([x.reshape(9, 63), torch.zeros(9, 1)], 1).double()
    layers = fold_iknet(loaded)
    assert len(layers) == 7 and layers[0][0].shape == (256, 64) and layers[-1][0].shape == (64, 256)
    for w, b, s, sh, act in layers:
        h = h @ w.double().T + b.double()
        if s is not None:
            h = h * s.double() + sh.double()
        if act == 1:
            h = torch.relu(h)
    np.testing.assert_allclose(h.numpy(), ref.numpy(), rtol=0, atol=2e-5 * float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ the CodaLab dump
class _Model:
    def __init__(self, joints):
        self.joints = joints

    def eval(self):
        pass

    def __call__(self, batch):
        return {"HybridBaseline": {"joints_3d_abs": self.joints[batch["idx"]].clone()}}


class _Fitter:
    """Stands in for FittingUnit: deterministic meshes from the joints it is given."""

    def __init__(self):
        self.calls = 0

    def __call__(self, inp, pred_joints):
        self.calls += 1
        pj = pred_joints.cpu().numpy()
        B = pj.shape[0]
        verts = [np.tile(pj[b, :1], (778, 1)) + 1e-3 * np.arange(778 * 3).reshape(778, 3) for b in range(B)]
        joints = [pj[b] + 0.01 for b in range(B)]
        return verts, joints


def _run(tmp_path, name, cfg, joints):
    from artiboost_amd.submit import HOSubmitEpochPass
    batches = [{"idx": slice(0, 3)}, {"idx": slice(3, 5)}]
    path = str(tmp_path / f"{name}.json")
    sp = HOSubmitEpochPass(dict(cfg, DUMP=True))
    sp(0, batches, _Model(joints), None, None, 0, path)
    return json.load(open(path)), sp


def test_submit_dump_with_fitted_meshes(tmp_path):
    """hodata_submit_epoch_pass.py:106-153: fitted vertices appended as they are (no flip); with use_fitted_joints the fitted joints
    with the reorder undone and y, z negated; otherwise the joints path is exactly that of a pass without fitting."""
    from artiboost_amd.submit import HOSubmitEpochPass
    joints = torch.randn(5, 21, 3, generator=torch.Generator().manual_seed(1))
    (xyz0, verts0), _ = _run(tmp_path, "plain", {}, joints)
    assert not np.asarray(verts0).any()
    fitter = _Fitter()
    (xyz1, verts1), sp1 = _run(tmp_path, "fit", {"FIT_MESH": True, "FITTING_UNIT": fitter}, joints)
    assert fitter.calls == 2 and sp1.fit_mesh_ik == "iknet"
    assert xyz1 == xyz0                                  # the joints path untouched
    want_v = np.stack(_Fitter()(None, joints)[0])
    assert np.asarray(verts1).shape == (5, 778, 3)
    np.testing.assert_allclose(np.asarray(verts1), want_v, rtol=0, atol=6e-6)
    (xyz2, verts2), _ = _run(tmp_path, "fitj", {"FIT_MESH": True, "FIT_MESH_USE_FITTED_JOINTS": True, "FIT_MESH_IK": "iksolver",
                                                "FITTING_UNIT": _Fitter()}, joints)
    assert verts2 == verts1
    _, unorder = HOSubmitEpochPass.get_order_idxs()
    fj = joints.numpy() + 0.01
    want_j = fj[:, unorder].copy()
    want_j[:, :, 1:] *= -1
    np.testing.assert_allclose(np.asarray(xyz2), want_j, rtol=0, atol=6e-6)          # 5 decimals


def test_fit_mesh_without_a_device_fails_with_a_clear_message(monkeypatch):
    from artiboost_amd.submit import HOSubmitEpochPass
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP device"):
        HOSubmitEpochPass({"FIT_MESH": True})


def test_draw_is_warned_about_once_and_fitting_goes_on():
    from artiboost_amd.submit import HOSubmitEpochPass
    with pytest.warns(UserWarning, match="postprocess_draw"):
        sp = HOSubmitEpochPass({"FIT_MESH": True, "DRAW": True, "FITTING_UNIT": _Fitter()})
    assert sp.fit_mesh


def test_reference_import_paths_of_the_fitting_module():
    from anakin.postprocess.iknet.fittingunit import FittingUnit
    from anakin.postprocess.iknet.model import IKNet
    from artiboost_amd import fitting
    assert FittingUnit is fitting.FittingUnit and IKNet is fitting.IKNet
