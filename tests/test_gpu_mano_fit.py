"""ab_mano_fit and the fitting path of the submit pass on the device, against tests/fit_oracle.py (the reference's fit restated in
torch with autograd and the JAX Adam, itself pinned to the reference's fittingunit.py by tests/golden/mano_fit.npz):

  iknet        the 7 ab_linear_fused launches against the float64 eval forward, within the first-order fp32 bound of the layers
  one step     teacher-forced: every step k of the float64 trajectory restarted on the device from the oracle's state; gradient and
               new parameters against the float64 values, within K x the spread the float32 oracle shows at the same state (per
               hand, or the batch-median relative spread times the hand's scale where that is larger)
  full fit     20 steps for B in {1, 37, 64, 100}: fitted joints and vertices within K x the float32 oracle's deviation from float64
               (this also covers the epilogue posing the mesh on J_regressor . v_shaped in fp32 while the steps use the float64-formed
               J_template / J_shapedirs: both are fp32 roundings of the same joints)
  batch mean   one hand fitted inside two batches: each result matches its own batch's oracle, and the two differ
  determinism  two launches give the same bits
  end to end   train/submit_reload.py --postprocess_fit_mesh on the clasbased eval config writes real vertices (subprocesses under a
               timeout)

K = 10 throughout: the device's result may be up to ten times as far from float64 as a float32 run of the reference's arithmetic
(the precision the reference itself runs in) is; the measured values are printed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fit_oracle as fo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
K_SPREAD = 10.0


def _hand():
    from artiboost_amd.fitting import mano_fit_tables
    from artiboost_amd.hpregnet import load_hand_model
    hm = load_hand_model(None)
    return hm, mano_fit_tables(hm, "cuda")


def _state(B, seed):
    """Seeded raw quaternions [B,64] and predicted joints [B,21,3] (float32): a hand-sized random skeleton around a root."""
    g = torch.Generator().manual_seed(seed)
    quat = torch.randn(B, 64, generator=g)
    quat.view(B, 16, 4)[:, :, 0] += 2.0
    pj = 0.03 * torch.randn(B, 21, 3, generator=g) + torch.tensor([0.0, 0.0, 0.6])
    return quat.contiguous(), pj.contiguous()


def _dev_fit(quat, pj, tables, **kw):
    from artiboost_amd import kernels as K
    o = K.mano_fit(quat.cuda(), pj.cuda(), tables, **kw)
    torch.cuda.synchronize()
    return {k: (v.cpu().double() if v is not None else None) for k, v in o.items()}


def _inf(a):
    return a.reshape(a.shape[0], -1).abs().amax(1)


# ------------------------------------------------------------------------------------------------ IKNet
def test_iknet_on_the_device_within_the_fp32_bound():
    from artiboost_amd.fitting import IKNet, IKNetHIP, fold_iknet, root_bone_target
    torch.manual_seed(2)
    net = IKNet()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.uniform_(-0.2, 0.2)
            m.running_var.uniform_(0.5, 2.0)
    net.eval()
    _, pj = _state(100, seed=5)
    _, _, inp = root_bone_target(pj)
    dev = IKNetHIP("cuda")
    dev.load_state_dict(net.state_dict())
    out = dev(inp.cuda()).cpu().double()
    # float64 forward of the folded fp32 layers (what the device evaluates) with the first-order fp32 bound of each layer:
    # |W| err_in |s| + (K + 2) u |W| |x| |s| + a few u of the output
    h = torch.cat([inp.reshape(100, 63), torch.zeros(100, 1)], 1).double()
    err = torch.zeros_like(h)
    for w, b, s, sh, act in fold_iknet(net.state_dict()):
        w, b = w.double(), b.double()
        s = s.double() if s is not None else torch.ones(w.shape[0], dtype=torch.float64)
        sh = sh.double() if sh is not None else torch.zeros(w.shape[0], dtype=torch.float64)
        y = (h @ w.T + b) * s + sh
        err = ((err @ w.abs().T) + (w.shape[1] + 2) * U * (h.abs() @ w.abs().T + b.abs())) * s.abs() + 3 * U * (y.abs() + sh.abs())
        h = torch.relu(y) if act == 1 else y
    with torch.no_grad():
        ref = net.double()(inp.double()).reshape(100, 64)
    # the fold itself (fp32 scale / shift) moves the float64 forward by a few fp32 roundings
    np.testing.assert_allclose(h.numpy(), ref.numpy(), rtol=0, atol=1e-5 * float(ref.abs().max()))
    ratio = float(((out - h).abs() / err).max())
    print(f"iknet: worst |device - float64| / fp32 bound = {ratio:.3f}")
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ teacher-forced steps
def test_teacher_forced_single_steps_match_float64():
    hm, tables = _hand()
    B = 64
    quat, pj = _state(B, seed=11)
    r64 = fo.fit(quat.double(), pj.double(), hm, n_iter=20)
    mano32 = fo.Mano(hm, torch.float32)
    so3_32, root32, _, tgt32 = fo.prepare(quat, pj, torch.float32)
    so3_64, root64, tgt64 = r64["so3_init"], r64["root"], r64["target"]
    excluded, worst_g, worst_x = 0, 0.0, 0.0
    for k, (x, m, v, _, _) in enumerate(r64["traj"]):
        n = k + 1
        state32 = (x.float(), m.float(), v.float())
        dev = _dev_fit(quat, pj, tables, n_iter=1, step0=n, state=state32, want_mesh=False, want_grad=True)
        # the float64 step and a float32 oracle step from the SAME (float32-rounded) state
        xs, ms, vs = (t.double() for t in state32)
        g64s, _ = fo.grad(xs, so3_64, root64, tgt64, r64["mano"])
        x64n, _, _ = fo.adam_step(xs, g64s, ms, vs, n)
        g32, _ = fo.grad(state32[0], so3_32, root32, tgt32, mano32)
        x32n, _, _ = fo.adam_step(state32[0], g32, state32[1], state32[2], n)
        kink = fo.near_kink(xs, root64, tgt64, r64["mano"], rel=1e-5)
        excluded += int(kink.sum())
        keep = ~kink
        # the float32 oracle's error at one hand is a single sample (it varies 100x between hands at the same step), so each
        # hand's bound is K x the larger of its own float32 error and the batch-median relative float32 error times its scale
        eg, eg32, sg = _inf(dev["grad"] - g64s), _inf(g32.double() - g64s), _inf(g64s)
        bound_g = K_SPREAD * torch.maximum(eg32, (eg32 / sg).median() * sg) + 64 * U * sg
        ex, ex32, sx = _inf(dev["params"] - x64n), _inf(x32n.double() - x64n), _inf(x64n - xs)
        bound_x = K_SPREAD * torch.maximum(ex32, (ex32 / sx).median() * sx) + 8 * U * _inf(x64n)
        worst_g = max(worst_g, float((eg / bound_g)[keep].max()))
        worst_x = max(worst_x, float((ex / bound_x)[keep].max()))
        assert (eg <= bound_g)[keep].all(), (k, float((eg / bound_g)[keep].max()))
        assert (ex <= bound_x)[keep].all(), (k, float((ex / bound_x)[keep].max()))
    print(f"teacher-forced: 20 steps x {B} hands, {excluded} hand-steps excluded near a kink; worst error / bound: grad {worst_g:.3f}, "
          f"params {worst_x:.3f}")
    assert excluded <= 0.05 * 20 * B


# ------------------------------------------------------------------------------------------------ the whole fit
@pytest.mark.parametrize("B", [1, 37, 64, 100])
def test_full_fit_within_the_float32_spread(B):
    hm, tables = _hand()
    quat, pj = _state(B, seed=100 + B)
    dev = _dev_fit(quat, pj, tables, n_iter=20, step0=1, want_loss=True)
    r64 = fo.fit(quat.double(), pj.double(), hm, n_iter=20)
    r32 = fo.fit(quat, pj, hm, n_iter=20, dtype=torch.float32)
    for key in ("joints", "verts"):
        e = float((dev[key] - r64[key]).abs().max())
        e32 = float((r32[key].double() - r64[key]).abs().max())
        print(f"B={B} {key}: device - float64 {e:.3e} m, float32 oracle - float64 {e32:.3e} m")
        assert e <= K_SPREAD * e32 + 1e-6, (key, e, e32)
    # the loss trace is the objective before each step
    errs = torch.stack([t[4] for t in r64["traj"]], 1)
    np.testing.assert_allclose(dev["loss"][:, 0].numpy(), errs[:, 0].numpy(), rtol=1e-3)
    # fitted joint 4 (thumb tip) is fitted vertex 745
    np.testing.assert_allclose(dev["joints"][:, 4].numpy(), dev["verts"][:, 745].numpy(), rtol=0, atol=1e-6)


def test_pose_regulariser_uses_the_whole_batch():
    hm, tables = _hand()
    qa, pa = _state(8, seed=21)
    qb, pb = _state(12, seed=22)
    qb[0], pb[0] = qa[0], pa[0]                          # hand 0 in both batches
    outs = []
    for q, p in ((qa, pa), (qb, pb)):
        dev = _dev_fit(q, p, tables)
        r64 = fo.fit(q.double(), p.double(), hm)
        r32 = fo.fit(q, p, hm, dtype=torch.float32)
        e = float((dev["verts"][0] - r64["verts"][0]).abs().max())
        e32 = float((r32["verts"][0].double() - r64["verts"][0]).abs().max())
        assert e <= K_SPREAD * e32 + 1e-6, (e, e32)
        outs.append(dev["verts"][0])
    assert float((outs[0] - outs[1]).abs().max()) > 1e-5


def test_fit_is_bit_reproducible():
    _, tables = _hand()
    quat, pj = _state(100, seed=31)
    a = _dev_fit(quat, pj, tables, want_loss=True, want_grad=True)
    b = _dev_fit(quat, pj, tables, want_loss=True, want_grad=True)
    for k in ("params", "m", "v", "verts", "joints", "loss", "grad"):
        assert torch.equal(a[k], b[k]), k


def test_fitting_unit_returns_the_reference_lists():
    from artiboost_amd.fitting import FittingUnit
    fu = FittingUnit(reload_prefix=None)
    _, pj = _state(5, seed=41)
    v, j = fu({}, pj.cuda())
    assert len(v) == len(j) == 5 and v[0].shape == (778, 3) and j[0].shape == (21, 3)
    np.testing.assert_allclose(np.stack(j)[:, 9], pj[:, 9].numpy(), rtol=0, atol=1e-6)     # moved to the predicted root


# ------------------------------------------------------------------------------------------------ the submit script
def _submit(tmp_path, extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "train", "submit_reload.py"), "--cfg",
                          os.path.join(ROOT, "config", "eval_ho3dv2_clasbased_artiboost_mi355x.yaml"), "--ignore_pretrained",
                          "--random_frames", "40", "--batch_size", "16", "--submit_dump"] + extra,
                         capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    exp = os.path.join(tmp_path, "exp", os.listdir(tmp_path / "exp")[0])
    js = [f for f in os.listdir(exp) if f.endswith("_SUBMIT.json")]
    assert len(js) == 1 and os.path.exists(os.path.join(exp, js[0].replace(".json", ".zip")))
    return json.load(open(os.path.join(exp, js[0])))


def test_submit_script_writes_fitted_vertices(tmp_path):
    from artiboost_amd.submit import HOSubmitEpochPass
    for d in "abc":
        (tmp_path / d).mkdir()
    xyz0, verts0 = _submit(tmp_path / "a", [])
    xyz1, verts1 = _submit(tmp_path / "b", ["--postprocess_fit_mesh"])
    xyz2, verts2 = _submit(tmp_path / "c", ["--postprocess_fit_mesh", "--postprocess_fit_mesh_use_fitted_joints"])
    v1 = np.asarray(verts1)
    assert v1.shape == (40, 778, 3) and (np.abs(v1).reshape(40, -1).max(1) > 0).all()
    assert not np.asarray(verts0).any()
    assert xyz1 == xyz0                                   # joints unchanged when fitted joints are off
    assert verts2 == verts1
    reorder, _ = HOSubmitEpochPass.get_order_idxs()
    fj4 = np.asarray(xyz2)[:, reorder[4]] * np.array([1.0, -1.0, -1.0])    # joint 4 before the dump transform
    np.testing.assert_allclose(fj4, v1[:, 745], rtol=0, atol=2e-5)
