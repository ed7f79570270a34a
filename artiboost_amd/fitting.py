"""Hand-mesh fitting of the submission pass on the device: anakin/postprocess/iknet/{fittingunit,model,checkpoints}.py.

The reference turns the predicted joints of a batch into MANO meshes (the vertex half of the HO3D CodaLab file) in two stages:
an IK network (`IKNet`, an MLP with eval-mode BatchNorm1d) gives an initial pose per hand, then 20 JAX Adam steps per hand fit
MANO to the joints, one hand at a time in a Python loop.  Here IKNet is 7 `ab_linear_fused` launches (BatchNorm folded into a
per-column affine, K zero-padded 63 -> 64) and the whole fit -- quaternion to axis-angle, the batch-mean pose regulariser, the
20 steps with their exact gradients, the final 778-vertex skinning -- is ONE `ab_mano_fit` launch for all hands of the batch.

Weights: `assets/postprocess/iknet.pt` (a download, `CheckpointIO` format `{"model": state_dict}`) when present, else a seeded
stand-in -- the rule `hpregnet.load_hand_model` applies to the MANO file.  The fit needs a HIP device; there is no CPU path."""
import os

import numpy as np
import torch
import torch.nn as nn

from . import kernels as K
from .hpregnet import load_hand_model
from .refiner import RefineNet, linear_fused

HIDDEN = [256, 512, 1024, 1024, 512, 256]


class IKNet(nn.Module):
    """postprocess/iknet/model.py:6-35 layer for layer (the state-dict keys of iknet.pt).  `forward` returns the RAW quaternions
    [B,16,4]; the reference's normalisation and axis-angle conversion (utils.py:13-41) run inside ab_mano_fit."""

    def __init__(self, njoints=21, hidden_size_pose=HIDDEN):
        super().__init__()
        neurons = [3 * njoints] + list(hidden_size_pose)
        layers = []
        for i, o in zip(neurons[:-1], neurons[1:]):
            layers += [nn.Linear(i, o), nn.BatchNorm1d(o), nn.ReLU()]
        layers.append(nn.Linear(neurons[-1], 16 * 4))
        self.invk_layers = nn.Sequential(*layers)

    def forward(self, joint):
        return self.invk_layers(joint.contiguous().view(-1, 63)).view(-1, 16, 4)


def load_iknet_checkpoint(path):
    """CheckpointIO(prefix, model=iknet).load("iknet.pt") (checkpoints.py:27-55): the file holds {"model": state_dict}; keys
    containing "mano_layer" are dropped before loading."""
    ck = torch.load(path, map_location="cpu", weights_only=False)
    return {k: v for k, v in ck["model"].items() if "mano_layer" not in k}


def fold_iknet(sd, eps=1e-5):
    """IKNet's state dict -> 7 (w [N,K], bias, scale, shift, act) for ab_linear_fused (CPU tensors): eval BatchNorm1d folded as
    RefineNet._fold does, the first layer's K zero-padded from 63 to 64, ReLU (act 1) on the six hidden layers."""
    out = []
    for li in range(7):
        w, b = sd[f"invk_layers.{3 * li}.weight"].float(), sd[f"invk_layers.{3 * li}.bias"].float()
        if li == 0:
            w = torch.cat([w, torch.zeros((w.shape[0], 1))], 1)
        if li < 6:
            s, sh = RefineNet._fold(sd, f"invk_layers.{3 * li + 1}", eps)
            out.append((w, b, s, sh, 1))
        else:
            out.append((w, b, None, None, 0))
    return out


class IKNetHIP:
    """IKNet in eval mode over device buffers: `load_state_dict` takes the reference's keys; `__call__(joint [B,21,3])` -> the raw
    quaternions [B,64] (7 ab_linear_fused launches)."""

    def __init__(self, device="cuda"):
        self.dev = torch.device(device)
        self.layers = None

    def load_state_dict(self, sd):
        self.layers = [tuple(t.contiguous().to(self.dev) if t is not None else None for t in l[:4]) + (l[4],) for l in fold_iknet(sd)]

    def __call__(self, joint):
        B = joint.shape[0]
        x = torch.zeros((B, 64), dtype=torch.float32, device=self.dev)
        x[:, :63] = joint.reshape(B, 63)
        for w, b, s, sh, act in self.layers:
            x = linear_fused(x, w, b, s, sh, act=act)
        return x


def mano_fit_tables(hand_model, device):
    """The MANO tables of ab_mano_fit on the device: those of ab_mano_lbs plus J_template = J_regressor . v_template [16,3] and
    J_shapedirs = J_regressor . shapedirs [16,3,10] (the joints are linear in beta; formed once in float64)."""
    f = {k: np.asarray(hand_model[k], np.float64) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
    f["J_template"] = f["J_regressor"] @ f["v_template"]
    f["J_shapedirs"] = np.einsum("jv,vcl->jcl", f["J_regressor"], f["shapedirs"])
    return {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(device) for k, v in f.items()}


def root_bone_target(pred_joints):
    """fittingunit.py:157-163: root = joint 9, bone = |joint 0 - joint 9|, the IKNet input (j - root) / bone."""
    root = pred_joints[:, 9:10]
    jc = pred_joints - root
    bone = torch.norm(jc[:, 0] - jc[:, 9], dim=1)
    return root, bone, jc / bone[:, None, None]


class FittingUnit:
    """postprocess/iknet/fittingunit.py:112-225 with the reference's constructor.  `hand_face_path` names the faces the reference
    reads for its OpenDR drawing only; fitting does not need it.  `__call__(inp, pred_joints)` -> (v_list, j_list) of numpy arrays
    [778,3] / [21,3] as the reference returns them; `fit(pred_joints)` -> device tensors [B,778,3], [B,21,3]."""

    def __init__(self, reload_prefix="assets/postprocess", hand_face_path="assets/postprocess/hand_close.npy",
                 mano_root="assets/mano_v1_2", device="cuda", n_iter=20, seed=1):
        if not torch.cuda.is_available():
            raise RuntimeError("--postprocess_fit_mesh fits the hand meshes on a HIP device (ab_mano_fit) and none is visible; "
                               "there is no CPU path")
        self.dev, self.n_iter = torch.device(device), n_iter
        self.reload_prefix, self.hand_face_path = reload_prefix, hand_face_path
        path = os.path.join(reload_prefix, "iknet.pt") if reload_prefix else None
        if path and os.path.isfile(path):
            sd = load_iknet_checkpoint(path)
        else:
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(seed)
                sd = IKNet().state_dict()
        self.iknet = IKNetHIP(device)
        self.iknet.load_state_dict(sd)
        self.tables = mano_fit_tables(load_hand_model(mano_root), self.dev)     # flat hand mean: hands_mean is not used

    def fit(self, pred_joints):
        pj = pred_joints.detach().to(self.dev, torch.float32).contiguous()
        _, _, inp = root_bone_target(pj)
        quat = self.iknet(inp)
        o = K.mano_fit(quat, pj, self.tables, n_iter=self.n_iter)
        return o["verts"], o["joints"]

    def __call__(self, inp, pred_joints):
        v, j = self.fit(pred_joints)
        B = v.shape[0]
        vj = torch.cat([v.reshape(B, -1), j.reshape(B, -1)], 1).cpu().numpy()      # one device-to-host copy per batch
        return list(vj[:, :778 * 3].reshape(B, 778, 3)), list(vj[:, 778 * 3:].reshape(B, 21, 3))
